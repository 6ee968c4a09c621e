// handle.cpp -- host side of libgbnns_hip.so, the C ABI declared in include/gbnns.h: the index handle (api_internal.h lists the other units).
//
// Owns device memory (index data in HBM, growable per-index workspaces: "lanes"), converts the reference's
// host-side data structures to the device layouts, and sequences the kernels of one batch call on
// one HIP stream -- the caller's, or with GBNNS_FLAG_DEFER_JOIN a lane's own, several batches in flight:
//     [MLP layer x3 + normalise] -> walk (first pass, fused re-rank) [-> retry pass] -> walk (general kernel,
//     hand-over list) [-> re-rank]
// There is no CPU fallback anywhere in this file: if HIP is unusable every entry point fails.

#include "api_internal.h"

#include <cmath>
#include <type_traits>

using namespace gbnns;
using namespace gbnns_api;

namespace gbnns_api {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

thread_local SlowLog g_slow;

// Host -> device copy of a caller's (pageable) array through the library's own page-locked staging buffer, in pieces.
// A plain hipMemcpy from pageable memory lets the runtime page-lock the caller's pages on the fly and remember the
// mapping; a caller that frees such an array and gets the same addresses back from its allocator for another one (numpy,
// std::vector) then has the next copy fault on the stale mapping now and then (round 4: "an illegal memory access" inside
// the first upload of gbnns_index_create, about one full test-suite run in three; never in a short run).  One-time
// uploads of an index do not miss the extra pass over host memory.
namespace {
std::mutex g_stage_mu;
void* g_stage = nullptr;  // two halves of kStagePiece bytes, page-locked, shared by h2d_staged and d2h_staged under g_stage_mu
constexpr size_t kStagePiece = 8u << 20;
}  // namespace

int h2d_staged(void* dst, const void* src, size_t bytes) {
    constexpr size_t kPiece = kStagePiece;
    std::lock_guard<std::mutex> lk(g_stage_mu);
    void*& stage = g_stage;
    if (!stage) HIP_TRY(hipHostMalloc(&stage, 2 * kPiece, hipHostMallocDefault));
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(hipEventCreateWithFlags(&ev[0], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ev[1], hipEventDisableTiming));
    int rc = GBNNS_OK;
    size_t done = 0;
    for (int i = 0; done < bytes && rc == GBNNS_OK; ++i, done += kPiece) {
        const size_t nb = std::min(kPiece, bytes - done);
        char* half = static_cast<char*>(stage) + (size_t)(i & 1) * kPiece;
        hipError_t e = i >= 2 ? hipEventSynchronize(ev[i & 1]) : hipSuccess;  // the piece that used this half has left it
        if (e == hipSuccess) {
            std::memcpy(half, static_cast<const char*>(src) + done, nb);
            e = hipMemcpyAsync(static_cast<char*>(dst) + done, half, nb, hipMemcpyHostToDevice, nullptr);
        }
        if (e == hipSuccess) e = hipEventRecord(ev[i & 1], nullptr);
        if (e != hipSuccess) rc = fail(GBNNS_ERR_HIP, "staged upload: %s", hipGetErrorString(e));
    }
    if (rc == GBNNS_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = fail(GBNNS_ERR_HIP, "staged upload: %s", hipGetErrorString(hipGetLastError()));
    (void)hipEventDestroy(ev[0]);
    (void)hipEventDestroy(ev[1]);
    return rc;
}

// The way back, for the same reason: device -> a caller's (pageable) array through the staging buffer, behind the work enqueued on s.
// Returns when the bytes are in dst.
int d2h_staged(void* dst, const void* src_dev, size_t bytes, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    if (!g_stage) HIP_TRY(hipHostMalloc(&g_stage, 2 * kStagePiece, hipHostMallocDefault));
    for (size_t done = 0; done < bytes; done += 2 * kStagePiece) {
        const size_t nb = std::min(2 * kStagePiece, bytes - done);
        HIP_TRY(hipMemcpyAsync(g_stage, static_cast<const char*>(src_dev) + done, nb, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(static_cast<char*>(dst) + done, g_stage, nb);
    }
    return GBNNS_OK;
}

// The per-call copies (declared in api_internal.h).  The caller's arrays of a long-lived process are exactly the arrays of the note
// above: numpy hands the addresses of a freed batch to the next one.  Met in the host path of gbnns_project at the end of a full
// test-suite run ("an illegal memory access", never in a short run), so pageable buffers no longer reach the runtime's copy calls.
namespace {
constexpr size_t kStageHalf = 2u << 20;
// The half to use next, free of the copy that used it last (host memcpy of one piece then runs beside the DMA of the piece before).
int lane_stage_half(Lane& L, char*& half, int& h) {
    if (!L.stage) {
        HIP_TRY(hipHostMalloc(&L.stage, 2 * kStageHalf, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&L.stage_ev[0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&L.stage_ev[1], hipEventDisableTiming));
    }
    h = L.stage_next;
    L.stage_next ^= 1;
    if (L.stage_busy[h]) HIP_TRY(hipEventSynchronize(L.stage_ev[h]));
    L.stage_busy[h] = false;
    half = static_cast<char*>(L.stage) + (size_t)h * kStageHalf;
    return GBNNS_OK;
}
}  // namespace

int host_copy_in(Lane& L, void* dst_dev, const void* src, size_t bytes, hipStream_t s) {
    if (bytes == 0) return GBNNS_OK;
    if (pinned_alias(static_cast<const char*>(src), bytes)) {
        HIP_TRY(hipMemcpyAsync(dst_dev, src, bytes, hipMemcpyHostToDevice, s));
        return GBNNS_OK;
    }
    for (size_t done = 0; done < bytes; done += kStageHalf) {
        const size_t nb = std::min(kStageHalf, bytes - done);
        char* half;
        int h;
        if (int rc = lane_stage_half(L, half, h)) return rc;
        std::memcpy(half, static_cast<const char*>(src) + done, nb);
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst_dev) + done, half, nb, hipMemcpyHostToDevice, s));
        HIP_TRY(hipEventRecord(L.stage_ev[h], s));
        L.stage_busy[h] = true;
    }
    return GBNNS_OK;
}

int host_copy_out(Lane& L, void* dst, const void* src_dev, size_t spitch, size_t width, size_t rows, hipStream_t s) {
    if (width == 0 || rows == 0) return GBNNS_OK;
    if (pinned_alias(static_cast<const char*>(dst), width * rows)) {
        if (spitch == width || rows == 1) HIP_TRY(hipMemcpyAsync(dst, src_dev, width * rows, hipMemcpyDeviceToHost, s));
        else HIP_TRY(hipMemcpy2DAsync(dst, width, src_dev, spitch, width, rows, hipMemcpyDeviceToHost, s));
        return GBNNS_OK;
    }
    if (spitch == width || rows == 1) {  // one contiguous run
        rows = width * rows;
        spitch = width = 1;
    }
    if (width > kStageHalf) return fail(GBNNS_ERR_INVALID, "host_copy_out: a row of %zu bytes", width);
    const size_t per = kStageHalf / width;  // rows per piece
    for (size_t r = 0; r < rows; r += per) {
        const size_t nr = std::min(per, rows - r);
        char* half;
        int h;
        if (int rc = lane_stage_half(L, half, h)) return rc;
        const char* from = static_cast<const char*>(src_dev) + r * spitch;
        if (width == 1) HIP_TRY(hipMemcpyAsync(half, from, nr, hipMemcpyDeviceToHost, s));
        else HIP_TRY(hipMemcpy2DAsync(half, width, from, spitch, width, nr, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::memcpy(static_cast<char*>(dst) + r * width, half, nr * width);
    }
    return GBNNS_OK;
}

int upload(DevBuf& dst, const void* src, size_t rows, size_t row_floats, size_t pad_floats,
           int mem_kind) {
    // copies a [rows x row_floats] f32 matrix into a zero-padded [rows x pad_floats] device matrix
    const size_t bytes = rows * pad_floats * sizeof(float);
    int rc = dst.ensure(bytes ? bytes : 4);
    if (rc) return rc;
    if (mem_kind == GBNNS_MEM_DEVICE) {
        if (pad_floats == row_floats) {
            HIP_TRY(hipMemcpy(dst.p, src, bytes, hipMemcpyDeviceToDevice));
        } else {
            HIP_TRY(hipMemset(dst.p, 0, bytes));
            HIP_TRY(hipMemcpy2D(dst.p, pad_floats * 4, src, row_floats * 4, row_floats * 4, rows, hipMemcpyDeviceToDevice));
        }
        return GBNNS_OK;
    }
    if (pad_floats == row_floats) return h2d_staged(dst.p, src, bytes);
    // padded rows: the rows are packed into a temporary device matrix first, then spread on the device
    DevBuf packed;
    if ((rc = packed.ensure(rows * row_floats * 4 ? rows * row_floats * 4 : 4))) return rc;
    rc = h2d_staged(packed.p, src, rows * row_floats * 4);
    hipError_t e = rc ? hipSuccess : hipMemset(dst.p, 0, bytes);
    if (!rc && e == hipSuccess) e = hipMemcpy2D(dst.p, pad_floats * 4, packed.p, row_floats * 4, row_floats * 4, rows, hipMemcpyDeviceToDevice);
    if (!rc && e == hipSuccess) e = hipDeviceSynchronize();
    packed.release();
    if (!rc && e != hipSuccess) rc = fail(GBNNS_ERR_HIP, "padded upload: %s", hipGetErrorString(e));
    return rc;
}

// [dout x (din+1)] rows = [W | b]  ->  W [dout x wstride] (zero padded) followed by bias [dout]
void repack_layer(const float* layer, uint32_t din, uint32_t dout, uint32_t wstride,
                  std::vector<float>& out) {
    const size_t base = out.size();
    out.resize(base + (size_t)dout * wstride + round_up(dout, 4), 0.f);  // keeps the next layer 16-B aligned
    float* w = out.data() + base;
    float* b = w + (size_t)dout * wstride;
    for (uint32_t o = 0; o < dout; ++o) {
        const float* row = layer + (size_t)o * (din + 1);
        std::memcpy(w + (size_t)o * wstride, row, (size_t)din * sizeof(float));
        b[o] = row[din];
    }
}

}  // namespace gbnns_api

// W [dout x wstride] (repack_layer's rows) -> the staged-order image of kernels.h, [slice][chunk][go b rows x ldw floats]: the
// one-launch projection's wavefronts copy a chunk of it into their staging buffers as it stands.  Once per index and form.
void gbnns::pack_net_image(const float* w, uint32_t wstride, uint32_t din, uint32_t dout, uint32_t b, uint32_t go, float* out) {
    const NetImageGeom g = net_image_geom(din, dout, b, go);
    const uint32_t k16 = round_up(din, 16);
    std::memset(out, 0, net_image_floats(din, dout, b, go) * sizeof(float));
    for (uint32_t s = 0; s < g.slices; ++s)
        for (uint32_t c = 0; c < g.nch; ++c) {
            float* chunk = out + ((size_t)s * g.nch + c) * g.buf;
            for (uint32_t r = 0; r < g.rows; ++r) {
                const uint32_t nr = g.interleaved ? (r % go) * b + r / go : r;   // the slice's neuron staged in row r
                const uint32_t o = std::min(s * g.rows + nr, dout - 1u);         // (rows beyond dout repeat the last: their results are dropped)
                for (uint32_t kk = 0; kk < g.ck; ++kk) {
                    const uint32_t k = c * g.ck + kk;
                    if (k >= k16) break;                                         // zeros from the row's padded end on
                    const uint32_t q = (kk >> 2) & 3u, t = kk & 3u;
                    chunk[(size_t)r * g.ldw + (kk & ~15u) + 4u * t + 2u * (q >> 1) + (q & 1u)] = w[(size_t)o * wstride + k];
                }
            }
        }
}

namespace gbnns_api {

// CSR (host) -> padded adjacency.  Order inside each list is preserved.  A neighbour id that
// repeats inside one list is dropped after its first occurrence: the reference would find it
// already visited (search_function.h:25), so this changes nothing observable.
int build_ell(const uint64_t* off, const uint32_t* nbr, uint64_t n, std::vector<uint32_t>& ell,
              uint32_t& stride) {
    uint64_t maxdeg = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (off[i + 1] < off[i]) return fail(GBNNS_ERR_INVALID, "graph_offsets not monotone at %llu",
                                             (unsigned long long)i);
        maxdeg = std::max<uint64_t>(maxdeg, off[i + 1] - off[i]);
    }
    if (maxdeg > (1u << 20)) return fail(GBNNS_ERR_UNSUPPORTED, "max degree %llu too large",
                                         (unsigned long long)maxdeg);
    stride = round_up((uint32_t)std::max<uint64_t>(maxdeg, 1), 16);
    if ((double)n * stride * 4.0 > 200e9)
        return fail(GBNNS_ERR_UNSUPPORTED, "padded adjacency would need %.1f GB", n * stride * 4e-9);
    ell.assign((size_t)n * stride, kInvalidId);
    std::vector<uint32_t> tmp;
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t* src = nbr + off[i];
        const uint32_t deg = (uint32_t)(off[i + 1] - off[i]);
        uint32_t* dst = ell.data() + (size_t)i * stride;
        bool dup = false;
        for (uint32_t j = 0; j < deg; ++j) {
            if (src[j] >= n) return fail(GBNNS_ERR_INVALID, "node %llu: neighbour id %u >= n",
                                         (unsigned long long)i, src[j]);
        }
        if (deg > 1) {
            tmp.assign(src, src + deg);
            std::sort(tmp.begin(), tmp.end());
            dup = std::adjacent_find(tmp.begin(), tmp.end()) != tmp.end();
        }
        if (!dup) {
            std::memcpy(dst, src, (size_t)deg * 4);
        } else {
            uint32_t m = 0;
            for (uint32_t j = 0; j < deg; ++j) {
                bool seen = false;
                for (uint32_t l = 0; l < m && !seen; ++l) seen = dst[l] == src[j];
                if (!seen) dst[m++] = src[j];
            }
        }
    }
    return GBNNS_OK;
}

// Diagnostic knobs.  The environment gives the process-wide defaults (read once when the library loads), gbnns_debug_knob changes
// them; a handle copies the defaults when it is created and from then on has its own (gbnns_index_knob) -- round 6: until then they were
// fourteen process-global atomics and a test that flipped one changed every handle of the process.  Results never depend on them.
//   "quotient"      0 = never the quotient form of the visited set (GBNNS_QUOTIENT)
//   "vs_disp"       probe number at which a probe sequence of that form gives up, 1 .. 15 (GBNNS_DEBUG_VS_DISP; 15 = the product's)
//   "max_waves"     most first-pass wavefronts per CU the LDS shares are cut for (GBNNS_MAX_WAVES; 0 = the per-kernel defaults)
//   "spec_min_nq"   smallest batch whose ef <= 64 first pass requests the rows before the visited test (walk_hot_spec_kernel;
//                   GBNNS_SPEC_MIN_NQ; 0 = never)
//   "spec_any_form" 1: ... whatever the form of the visited set (tests; default: only tables NOT in the quotient form)
//   "mlp_small"     smallest batch IN FLIGHT whose hidden projection layers run on the small-footprint kernel (0 = never)
//   "mlp_net"       0 = never the one-launch projection (mlp_net.hip), 1 = for the shapes and batch sizes it serves, in the form
//                   run_project's rule picks, 2 = always its whole-CU form, 3 = its half-CU form wherever that fits (GBNNS_MLP_NET)
//   "mlp_net_form"  (read only, gbnns_index_knob_get) the form the handle's last one-launch projection ran in: 0 = whole-CU blocks,
//                   1 = half-CU blocks, -1 = none yet
//   "cus"           (read only) the compute units of the handle's device: what the projection's launch rules count rounds of the machine in
//   "mlp_slab"      0 = never the slab kernel for single layers (mlp_net.hip, mlp_slab_kernel), 1 = where a layer is one round of it
//   "late_rows"     generic two-list kernels over 192- / 256- / 576-byte rows -- -1 = by shape and residency (call_plan.cpp), 0 = rows
//                   requested before the visited test, 1 = after it (GBNNS_LATE_ROWS)
//   "spec_tail"     largest partial last round of a lone launch, in percent of the device's wavefront slots, whose wavefronts request
//                   their rows before the visited test (0 = off)
//   "byte_query_int" gbnns_search_byte_queries: the beam classes whose byte-walk first pass is the integer instance (walk_bytes_q.hip) -- a mask,
//                   bit 0 = one list register (ef <= 64), bit 1 = two (ef <= 128), bit 2 = the two-list kernel (ef <= 1 024); 0 = never: the call
//                   is served by walk_bytes.hip on the widened queries (A/B runs; GBNNS_BYTE_QUERY_INT).  Default: kByteQueryIntDefault
//   "half_walk_fast" GBNNS_FLAG_HALF_WALK: 0 = the general kernel's half-walk instance takes the whole batch also where walk_half_base.hip has an
//                   instance; 1 (default) = the fast instances of the dimension classes the measurement rule has kept (walk_plan.cpp); 2 = every
//                   fast instance the unit has (tools/half_walk_timing.py measures the three against each other; the tests run the unkept
//                   instances with 2 and the general instance on the fast shapes with 0; GBNNS_HALF_WALK_FAST)
//   "gather_budget" gbnns_index_exact_knn_gather: list entries (4 bytes each) the id lists of one round may hold together; default 2^26 (256 MiB),
//                   and the call never takes less than n.  Not for tuning: a test forces several rounds at a few thousand rows with it
//   "gather_timing" 1 = a gathered call times its stages with events (its rounds then run one after the other); read back with
//                   gbnns_index_knob_get: "gather_census_us", "gather_fill_us", "gather_scan_us", "gather_rounds" (tools/exact_gather_timing.py)
//   "coop"          the two-wavefront walk for small batches (walk_coop.hip): -1 = where it serves and the batch leaves the room
//                   (default), 0 = never, 1 = wherever the shape allows (tests, A/B runs; GBNNS_COOP)
//   "order_min"     smallest batch of a NET / LOWQ search over at least 16 walked coordinates that is walked in locality order
//                   (search_core.cpp, gd_order.hip); 0 = never, negative values count as 0 (GBNNS_ORDER_MIN; default 32 768)
//   "order_bits"    width of that order's key, the sign bits of the first coordinates: 10 .. 16, clamped (GBNNS_ORDER_BITS; default 12)
//   "order_last"    (read only) queries the handle's last search call walked in locality order: its batch size, or 0 when it was not
//                   ordered; gbnns_index_order_last copies the permutation of the last call that was
// Process-wide only (gbnns_exact_knn has no handle):
//   "hot"            0 = the generic register-list / two-list instances also where the plan has a walk_hot* / walk_reg_wide instance
//                    (GBNNS_HOT; A/B runs: the instance family a tagged call's kernels are built from, untagged)
//   "knn_chunk"      most rows per filtered chunk (a multiple of 64)
//   "knn_pool_min_k" shortest list gbnns_exact_knn keeps as an unordered pool (one wavefront per query and chunk) instead of a heap
//                    (measured on 10^6 x 32: k = 48 0.327 against 0.333 s, k = 100 0.425 against 0.536 s, k = 1 000 2.4 against 7.6 s)
//   "knn_filter"     0 = gbnns_exact_knn without the matrix-core filter (GBNNS_KNN_FILTER; tests compare the two paths)
//   "knn_slab"       0 = queries in slabs whose key lists take at most 4 GiB (default); v > 0: at most max(128, v & ~127) queries a slab
//                    (tests: several slabs at a few hundred queries; gbnns_debug_knn_slab reports the slab of a shape)
// The classes where the integer first pass measured faster than the float byte walk plus the widening kernel by more than the baseline's
// run-to-run spread (profiles/byte_query_timing.txt)
constexpr int kByteQueryIntDefault = 7;
int knob_env(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
bool knob_set(Knobs& k, const char* name, int value) {
    if (!std::strcmp(name, "quotient")) k.quotient = value != 0;
    else if (!std::strcmp(name, "vs_disp")) k.vs_disp = value <= 0 ? 15 : std::min(15, value);
    else if (!std::strcmp(name, "max_waves")) k.max_waves = std::max(0, std::min(32, value));
    else if (!std::strcmp(name, "spec_any_form")) k.spec_any_form = value != 0;
    else if (!std::strcmp(name, "spec_min_nq")) k.spec_min_nq = std::max(0, value);
    else if (!std::strcmp(name, "mlp_small")) k.mlp_small = std::max(0, value);
    else if (!std::strcmp(name, "mlp_net")) k.mlp_net = std::max(0, std::min(3, value));
    else if (!std::strcmp(name, "mlp_slab")) k.mlp_slab = std::max(0, std::min(2, value));
    else if (!std::strcmp(name, "late_rows")) k.late_rows = std::max(-1, std::min(1, value));
    else if (!std::strcmp(name, "spec_tail")) k.spec_tail = std::max(0, std::min(100, value));
    else if (!std::strcmp(name, "coop")) k.coop = std::max(-1, std::min(1, value));
    else if (!std::strcmp(name, "hot")) k.hot = value != 0;
    else if (!std::strcmp(name, "byte_query_int")) k.byte_query_int = std::max(0, std::min(7, value));
    else if (!std::strcmp(name, "half_walk_fast")) k.half_walk_fast = std::max(0, std::min(2, value));
    else if (!std::strcmp(name, "gather_budget")) k.gather_budget = std::max(1, value);
    else if (!std::strcmp(name, "gather_timing")) k.gather_timing = value != 0;
    else if (!std::strcmp(name, "order_min")) k.order_min = std::max(0, value);
    else if (!std::strcmp(name, "order_bits")) k.order_bits = std::max(10, std::min(16, value));
    else return false;
    return true;
}
static std::mutex g_knob_mu;
static Knobs& knob_default_ref() {  // (function-local: initialised on first use, whatever the order of the static initialisers)
    static Knobs d = [] {
        Knobs k{};
        knob_set(k, "quotient", knob_env("GBNNS_QUOTIENT", 1));
        knob_set(k, "vs_disp", knob_env("GBNNS_DEBUG_VS_DISP", 15));
        knob_set(k, "max_waves", knob_env("GBNNS_MAX_WAVES", 0));
        knob_set(k, "spec_min_nq", knob_env("GBNNS_SPEC_MIN_NQ", 32768));
        knob_set(k, "spec_any_form", knob_env("GBNNS_SPEC_ANY_FORM", 0));
        knob_set(k, "mlp_small", knob_env("GBNNS_MLP_SMALL", 4096));
        knob_set(k, "mlp_net", knob_env("GBNNS_MLP_NET", 1));
        knob_set(k, "mlp_slab", knob_env("GBNNS_MLP_SLAB", 1));
        knob_set(k, "late_rows", knob_env("GBNNS_LATE_ROWS", -1));
        knob_set(k, "spec_tail", knob_env("GBNNS_SPEC_TAIL", 50));
        knob_set(k, "coop", knob_env("GBNNS_COOP", -1));
        knob_set(k, "hot", knob_env("GBNNS_HOT", 1));
        knob_set(k, "byte_query_int", knob_env("GBNNS_BYTE_QUERY_INT", kByteQueryIntDefault));
        knob_set(k, "half_walk_fast", knob_env("GBNNS_HALF_WALK_FAST", 1));
        knob_set(k, "gather_budget", knob_env("GBNNS_GATHER_BUDGET", 1 << 26));
        knob_set(k, "gather_timing", 0);
        knob_set(k, "order_min", knob_env("GBNNS_ORDER_MIN", 32768));
        knob_set(k, "order_bits", knob_env("GBNNS_ORDER_BITS", 12));
        return k;
    }();
    return d;
}
Knobs knob_defaults() {
    std::lock_guard<std::mutex> g(g_knob_mu);
    return knob_default_ref();
}
std::atomic<int> g_knob_knn_chunk{std::max(64, knob_env("GBNNS_KNN_CHUNK", 1 << 15) & ~63)};  // (a multiple of 64, never 0: the chunk loops step by it)
std::atomic<int> g_knob_knn_pool_min_k{std::max(1, knob_env("GBNNS_KNN_POOL_MIN_K", 64))};
std::atomic<int> g_knob_knn_filter{knob_env("GBNNS_KNN_FILTER", 1)};
std::atomic<int> g_knob_knn_slab{0};

// (defined here, beside the defaults, so that gbnns_debug_knob below can reach them under the lock)
static bool knob_default_set(const char* name, int value) {
    std::lock_guard<std::mutex> g(g_knob_mu);
    return knob_set(knob_default_ref(), name, value);
}

}  // namespace gbnns_api

extern "C" {

int gbnns_version(void) { return GBNNS_VERSION; }

const char* gbnns_last_error(void) { return g_err.c_str(); }

int gbnns_device_count(void) {
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

void gbnns_free(void* p) { std::free(p); }

// gbnns_index_create (F32: the table is desc->db, `table` is ignored), gbnns_index_create_bytes and gbnns_index_create_half_base (`table`)
static int index_create(const gbnns_index_desc* desc, RowKind rows, const void* table, gbnns_index** out) {
    if (!desc || !out) return fail(GBNNS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (desc->struct_size != sizeof(gbnns_index_desc))
        return fail(GBNNS_ERR_INVALID, "gbnns_index_desc.struct_size mismatch (%u != %zu)",
                    desc->struct_size, sizeof(gbnns_index_desc));
    if (desc->n == 0 || desc->n >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "n must be in [1, 2^31)");
    const bool narrow = rows != RowKind::F32;  // rows of 1- or 2-byte elements, handed over beside the descriptor
    if (desc->d == 0 || (!narrow && !desc->db)) return fail(GBNNS_ERR_INVALID, "db / d missing");
    if (narrow) {
        const char *fn = row_create_fn(rows), *arg = row_table_arg(rows);
        if (desc->db) return fail(GBNNS_ERR_INVALID, "%s: desc->db must be NULL (the table is %s)", fn, arg);
        if (!table) return fail(GBNNS_ERR_INVALID, "%s: %s missing", fn, arg);
        if (desc->d_low == 0 || !desc->db_low)
            return fail(GBNNS_ERR_INVALID, "%s: d_low and db_low are required (a %s serves NET / LOWQ searches)", fn, row_handle_noun(rows));
    } else {
        table = desc->db;
    }
    if (!desc->graph_offsets || !desc->graph_nbrs) return fail(GBNNS_ERR_INVALID, "graph missing");
    if (desc->metric != GBNNS_METRIC_L2 && desc->metric != GBNNS_METRIC_NEG_DOT)
        return fail(GBNNS_ERR_INVALID, "unknown metric %d", desc->metric);
    if (desc->mem_kind != GBNNS_MEM_HOST && desc->mem_kind != GBNNS_MEM_DEVICE)
        return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", desc->mem_kind);
    if ((desc->d_low != 0) != (desc->db_low != nullptr))
        return fail(GBNNS_ERR_INVALID, "d_low and db_low must be given together");
    const bool has_net = desc->net_l1 || desc->net_l2 || desc->net_l3;
    if (has_net && !(desc->net_l1 && desc->net_l2 && desc->net_l3 && desc->d_hidden && desc->d_low))
        return fail(GBNNS_ERR_INVALID, "net needs all three layers, d_hidden and d_low");

    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(GBNNS_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
    if (desc->device < 0 || desc->device >= count)
        return fail(GBNNS_ERR_NO_DEVICE, "device %d out of range (%d devices)", desc->device, count);
    HIP_TRY(hipSetDevice(desc->device));

    gbnns_index* ix = new (std::nothrow) gbnns_index;
    if (!ix) return fail(GBNNS_ERR_OOM, "host allocation failed");
    ix->device = desc->device;
    ix->metric = desc->metric;
    ix->n = desc->n;
    ix->d = desc->d;
    ix->d_low = desc->d_low;
    ix->d_hidden = desc->d_hidden;
    (void)hipDeviceGetAttribute(&ix->cus, hipDeviceAttributeMultiprocessorCount, ix->device);
    ix->knob = knob_defaults();
    ix->rows = rows;
    ix->d_pad = row_pad(desc->d, rows);  // (elements of a row = floats of a staged re-rank query)
    ix->dl_pad = round_up(desc->d_low, 4);
    int rc = GBNNS_OK;

    auto take = [&](const float* src, uint32_t dim, uint32_t pad, DevBuf& own, const float*& dst) -> int {
        if (desc->mem_kind == GBNNS_MEM_DEVICE && pad == dim) {
            dst = src;  // borrowed: rows already 16-B aligned
            return GBNNS_OK;
        }
        int r = upload(own, src, ix->n, dim, pad, desc->mem_kind);
        dst = own.as<float>();
        return r;
    };
    // rows of 1- or 2-byte elements: [n x d] -> [n x d_pad], zero padded, in an exactly sized buffer; a DEVICE table already in that layout
    // (d_pad == d, a 16-byte aligned address) is borrowed
    auto take_packed = [&](DevBuf& own, const void*& dst) -> int {
        const size_t elem = row_elem_bytes(rows), d = ix->d * elem, pad = ix->d_pad * elem, n = ix->n;  // (bytes of a row)
        const bool device = desc->mem_kind == GBNNS_MEM_DEVICE;
        if (device && pad == d && (reinterpret_cast<uintptr_t>(table) & 15u) == 0) {
            dst = table;
            return GBNNS_OK;
        }
        const hipError_t ea = hipMalloc(&own.p, n * pad);
        if (ea != hipSuccess) {
            own.p = nullptr;
            return fail(GBNNS_ERR_OOM, "hipMalloc(%zu): %s", n * pad, hipGetErrorString(ea));
        }
        own.bytes = n * pad;
        dst = own.p;
        if (!device && pad == d) return h2d_staged(own.p, table, n * d);
        DevBuf packed;  // (HOST rows that need padding: packed on the device first, then spread)
        const void* src = table;
        int r = GBNNS_OK;
        if (!device) {
            if ((r = packed.ensure(n * d))) return r;
            r = h2d_staged(packed.p, table, n * d);
            src = packed.p;
        }
        hipError_t e = r ? hipSuccess : hipMemset(own.p, 0, n * pad);
        if (!r && e == hipSuccess) e = hipMemcpy2D(own.p, pad, src, d, d, n, hipMemcpyDeviceToDevice);
        if (!r && e == hipSuccess) e = hipDeviceSynchronize();
        packed.release();
        if (!r && e != hipSuccess) r = fail(GBNNS_ERR_HIP, "%s table upload: %s", rows == RowKind::U8 ? "byte" : "half", hipGetErrorString(e));
        return r;
    };
    if (narrow) {
        rc = take_packed(ix->base_own, ix->base);
    } else {
        const float* dst = nullptr;
        rc = take(static_cast<const float*>(table), ix->d, ix->d_pad, ix->base_own, dst);
        ix->base = dst;
    }
    if (!rc && desc->db_low) rc = take(desc->db_low, ix->d_low, ix->dl_pad, ix->db_low_own, ix->db_low);

    if (!rc) {
        std::vector<uint32_t> ell;
        rc = build_ell(desc->graph_offsets, desc->graph_nbrs, ix->n, ell, ix->ell_stride);
        if (!rc) rc = ix->ell.ensure(ell.size() * 4);
        if (!rc) {
            rc = h2d_staged(ix->ell.p, ell.data(), ell.size() * 4);
        }
    }

    if (!rc && has_net) {
        const uint32_t d = ix->d, dh = ix->d_hidden, dl = ix->d_low;
        std::vector<float> l1, l2, l3;
        const float *p1 = desc->net_l1, *p2 = desc->net_l2, *p3 = desc->net_l3;
        if (desc->mem_kind == GBNNS_MEM_DEVICE) {
            l1.resize((size_t)dh * (d + 1));
            l2.resize((size_t)dh * (dh + 1));
            l3.resize((size_t)dl * (dh + 1));
            hipError_t e = hipMemcpy(l1.data(), p1, l1.size() * 4, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(l2.data(), p2, l2.size() * 4, hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(l3.data(), p3, l3.size() * 4, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = fail(GBNNS_ERR_HIP, "net download: %s", hipGetErrorString(e));
            p1 = l1.data();
            p2 = l2.data();
            p3 = l3.data();
        }
        if (!rc) {
            // (rows padded with zeros to 16 floats: the one-launch projection reads whole 16-input blocks)
            ix->ws1 = round_up(d, 16);
            ix->ws2 = round_up(dh, 16);
            ix->ws3 = round_up(dh, 16);

            std::vector<float> packed;
            repack_layer(p1, d, dh, ix->ws1, packed);
            const size_t o2 = packed.size();
            repack_layer(p2, dh, dh, ix->ws2, packed);
            const size_t o3 = packed.size();
            repack_layer(p3, dh, dl, ix->ws3, packed);
            // the one-launch projection's staged-order images, one per form: built here, once, so that no search packs or waits
            size_t img_off[2][3];
            {
                const size_t wo[3] = {0, o2, o3};
                const uint32_t din[3] = {d, dh, dh}, dout[3] = {dh, dh, dl}, ws[3] = {ix->ws1, ix->ws2, ix->ws3};
                for (int form = 0; form < 2; ++form)
                    for (int l = 0; l < 3; ++l) {
                        const uint32_t b = l < 2 ? 8u : net_image_b3(dl), go = net_image_go(form);
                        img_off[form][l] = packed.size();
                        packed.resize(packed.size() + net_image_floats(din[l], dout[l], b, go));
                        pack_net_image(packed.data() + wo[l], ws[l], din[l], dout[l], b, go, packed.data() + img_off[form][l]);
                    }
            }
            rc = ix->net.ensure(packed.size() * 4);
            // (through the staging buffer like every other upload of a pageable array here -- `packed` is one, and a plain hipMemcpy from it
            // is the copy h2d_staged exists to avoid: "net upload: an illegal memory access" turned up once in a full test-suite run)
            if (!rc) rc = h2d_staged(ix->net.p, packed.data(), packed.size() * 4);
            float* base = ix->net.as<float>();
            ix->w1 = base;
            ix->b1 = ix->w1 + (size_t)dh * ix->ws1;
            ix->w2 = base + o2;
            ix->b2 = ix->w2 + (size_t)dh * ix->ws2;
            ix->w3 = base + o3;
            ix->b3 = ix->w3 + (size_t)dl * ix->ws3;
            for (int form = 0; form < 2; ++form)
                for (int l = 0; l < 3; ++l) ix->net_img[form][l] = base + img_off[form][l];
            ix->has_net = true;
        }
    }
    if (!rc) rc = ix->lanes[0].ctrl.ensure(512);
    if (!rc) {
        // (hipMemset on device memory may return before the fill has run: callers' streams may be non-blocking
        // ones that do not order themselves after the null stream, so wait for it here)
        hipError_t e = hipMemset(ix->lanes[0].ctrl.p, 0, 512);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) rc = fail(GBNNS_ERR_HIP, "ctrl init: %s", hipGetErrorString(e));
        ix->lanes[0].ctrl_ready = true;
    }
    if (rc) {
        gbnns_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return GBNNS_OK;
}

int gbnns_index_create(const gbnns_index_desc* desc, gbnns_index** out) { return index_create(desc, RowKind::F32, nullptr, out); }

int gbnns_index_create_bytes(const gbnns_index_desc* desc, const uint8_t* db_bytes, gbnns_index** out) {
    return index_create(desc, RowKind::U8, db_bytes, out);
}

int gbnns_index_is_bytes(const gbnns_index* ix) { return ix && ix->is(RowKind::U8) ? 1 : 0; }

int gbnns_index_create_half_base(const gbnns_index_desc* desc, const uint16_t* db_half, gbnns_index** out) {
    return index_create(desc, RowKind::F16, db_half, out);
}

int gbnns_index_is_half_base(const gbnns_index* ix) { return ix && ix->is(RowKind::F16) ? 1 : 0; }

int gbnns_index_set_aux_graph(gbnns_index* ix, const uint64_t* offsets, const uint32_t* nbrs) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // no search may still be reading the old table
    ix->has_aux = false;
    if (!offsets && !nbrs) return GBNNS_OK;
    if (!offsets || !nbrs) return fail(GBNNS_ERR_INVALID, "auxiliary graph: offsets / nbrs missing");
    std::vector<uint32_t> ell;
    int rc = build_ell(offsets, nbrs, ix->n, ell, ix->aux_stride);
    if (rc) return rc;
    if ((rc = ix->aux_ell.ensure(ell.size() * 4))) return rc;
    if (int rc2 = h2d_staged(ix->aux_ell.p, ell.data(), ell.size() * 4)) return rc2;
    ix->has_aux = true;
    return GBNNS_OK;
}

uint32_t gbnns_index_d_low(const gbnns_index* ix) { return ix ? ix->d_low : 0u; }
uint64_t gbnns_index_n(const gbnns_index* ix) { return ix ? ix->n : 0u; }
uint32_t gbnns_index_d(const gbnns_index* ix) { return ix ? ix->d : 0u; }
int gbnns_index_device(const gbnns_index* ix) { return ix ? ix->device : -1; }

int gbnns_index_destroy(gbnns_index* ix) {
    if (!ix) return GBNNS_OK;
    (void)hipSetDevice(ix->device);
    for (auto& pc : ix->pending)
        for (auto& e : pc.ev) (void)hipEventDestroy(e);
    (void)hipDeviceSynchronize();  // lanes may still be running a call whose join was deferred
    if (ix->order_ev) (void)hipEventDestroy(ix->order_ev);
    if (ix->fork_ev) (void)hipEventDestroy(ix->fork_ev);
    if (ix->prof_ctrl) (void)hipHostFree(ix->prof_ctrl);
    for (Lane& L : ix->lanes) {
        if (L.stats_ev) (void)hipEventDestroy(L.stats_ev);
        if (L.done_ev) (void)hipEventDestroy(L.done_ev);
        if (L.prev_ev) (void)hipEventDestroy(L.prev_ev);
        if (L.h_stats) (void)hipHostFree(L.h_stats);
        if (L.stage) (void)hipHostFree(L.stage);
        for (hipEvent_t e : L.stage_ev)
            if (e) (void)hipEventDestroy(e);
        if (L.stream) (void)hipStreamDestroy(L.stream);
        for (int i = 0; DevBuf* b = L.bufs(i); ++i) b->release();
    }
    DevBuf* bufs[] = {&ix->base_own, &ix->db_low_own, &ix->ell, &ix->aux_ell, &ix->net, &ix->net_mfma, &ix->low_half, &ix->low_r, &ix->tags};
    for (DevBuf* b : bufs) b->release();
    delete ix;
    return GBNNS_OK;
}

}  // extern "C"

namespace gbnns_api {


// What decides a projection's launches: the net's shape, the batch, the device's CU count, the call's flags, the handle's knobs and the
// ALIGNMENT of the buffers (x, w: never dereferenced here; the hidden activations live in 256-byte aligned scratch).
struct ProjShape {
    uint32_t d, dh, dl, dl_pad, nq, xstride;
    int cus;
    bool in_flight, mfma;
    int mlp_net, mlp_slab, mlp_small;
    const float* x;
    const float* w[3];
    uint32_t ws[3];
};
enum class ProjPath { Net, MfmaNet, Layers };
enum class LayerPath { Layer, Slab, Mfma };
struct ProjRoute {
    ProjPath path;
    int form;                // Net: kNetWholeCu / kNetHalfCu
    int small_footprint;     // Layers: LayerParams::small_footprint of the three
    LayerPath layer[3];
};

static NetLaunch net_of(const ProjShape& q) {
    NetLaunch n{};
    n.x = q.x; n.xstride = q.xstride; n.nq = q.nq; n.ostride = q.dl_pad; n.cus = q.cus;
    for (int l = 0; l < 3; ++l) { n.w[l] = q.w[l]; n.wstride[l] = q.ws[l]; }
    n.din[0] = q.d; n.din[1] = n.din[2] = q.dh;
    n.dout[0] = n.dout[1] = q.dh; n.dout[2] = q.dl;
    return n;
}

// layer l without its bias and output pointers; h: the hidden activations it reads (l > 0)
static LayerParams layer_of(const ProjShape& q, int l, int small_footprint, const float* h) {
    LayerParams p{};
    p.x = l ? h : q.x; p.xstride = l ? q.dh : q.xstride; p.w = q.w[l]; p.wstride = q.ws[l];
    p.nq = q.nq; p.din = l ? q.dh : q.d; p.dout = l < 2 ? q.dh : q.dl; p.ostride = l < 2 ? q.dh : q.dl_pad;
    p.relu = l < 2; p.normalize = l == 2; p.small_footprint = small_footprint;
    return p;
}

// The one place that says which kernels a projection runs on: the route run_project follows, and in `plan` (where asked for) the instance
// of every launch, from the same pick functions the launchers switch on.
static ProjRoute project_route(const ProjShape& q, ProjPlan* plan) {
    ProjRoute r{};
    ProjPlan none{};
    if (!plan) plan = &none;
    *plan = ProjPlan{};
    // the whole net in one launch where it serves (round 5, mlp_net.hip: 0.048 against 0.075 ms on the SIFT shape; the
    // round-2 one-launch form -- csrc/project.hip, deleted in round 4 -- was slower than the three launches)
    if (!q.mfma && q.mlp_net) {
        NetLaunch n = net_of(q);
        if (mlp_net_serves(n)) {
            // batches in flight: blocks of half a CU (4 wavefronts, <= 80 KB) -- one is placed as soon as a CU is half drained of the
            // other lanes' walk wavefronts, where a whole-CU block waits for all of them (profiles/half_cu_projection.txt: sift-like
            // 33.2 against 32.2 M queries/s); alone the whole-CU form is the faster one (50 against 62 us), so lone calls keep it
            const int mode = q.mlp_net;
            const bool want_half = mode == 3 || (mode == 1 && q.in_flight);
            n.form = want_half && mlp_net_half_serves(n) ? kNetHalfCu : kNetWholeCu;
            r.path = ProjPath::Net;
            r.form = n.form;
            NetPick k{};
            if (mlp_net_pick(n, &k)) plan->add(k.inst);
            return r;
        }
    }
    if (q.mfma && !getenv("GBNNS_MFMA_LAYERS") && mlp_mfma_net_serves(q.d, q.dh, q.dl)) {
        // the throughput option in one launch (round 6, mlp_mfma_net.hip); GBNNS_MFMA_LAYERS=1 keeps round 5's three launches (A/B)
        r.path = ProjPath::MfmaNet;
        MfmaNetPick k{};
        if (mlp_mfma_net_pick(net_of(q), &k)) plan->add(k.inst);
        return r;
    }
    r.path = ProjPath::Layers;
    // batches in flight whose walks fill the machine: the small-footprint kernel for the hidden layers (mlp.hip; sift-like
    // +2.5 % at ef 64, +3.6 % at ef 36; a 1 000-query GIST batch -- one walk wavefront per SIMD, nothing to squeeze in
    // beside -- and every batch that runs alone are faster on the big-tile kernel)
    const int small_min = q.mlp_small;
    // (... up to 32 times that: a 1 M-query DEEP batch is twenty rounds of the machine on its own, its projection is not
    // waiting for room, and the big-tile kernel's 12 % matter again: 43.1 against 41.5 M queries/s)
    r.small_footprint = (q.in_flight && small_min > 0 && q.nq >= (uint32_t)small_min && (uint64_t)q.nq <= 32ull * (uint64_t)small_min) ? 1 : 0;
    // a layer that is one round of the machine for the slab kernel (small batches, the GIST shape's 1 000 x 960 -> 1 024 -> 1 024 -> 64:
    // 117 against 153 us, the 64-neuron last layer alone 15 against 43) takes that; everything else the per-layer kernels of mlp.hip
    for (int l = 0; l < 3; ++l) {
        const LayerParams lp = layer_of(q, l, r.small_footprint, nullptr);
        LayerPick k{};
        // (batches in flight: only the narrow shape -- 35 KB, 256 threads -- finds room beside the other lanes' walk wavefronts; the
        // wide one's 103 KB workgroups wait for a CU to drain: GIST 2.27 against 2.58 M queries/s.  Knob value 2 = wide in flight too.)
        const int slab = q.mlp_slab;
        if (q.mfma) {
            r.layer[l] = LayerPath::Mfma;
            k = mlp_layer_mfma_pick(lp);
        } else if (!lp.small_footprint && slab && (!q.in_flight || lp.dout <= 64u || slab >= 2) && mlp_slab_wins(lp, q.cus)) {
            r.layer[l] = LayerPath::Slab;
            SlabPick sk{};
            if (mlp_slab_pick(lp, q.cus, 0, &sk)) { k.inst = sk.inst; k.normalize_after = sk.normalize_after; }
        } else {
            r.layer[l] = LayerPath::Layer;
            k = mlp_layer_pick(lp);
        }
        plan->add(k.inst);
        if (k.normalize_after && q.nq) {
            ProjInstance nrm{};
            nrm.family = ProjFamily::Normalize;
            plan->add(nrm);
        }
    }
    return r;
}

static ProjShape shape_of(const gbnns_index* ix, const float* x, uint32_t xstride, uint32_t nx, bool in_flight, bool mfma) {
    ProjShape q{};
    q.d = ix->d; q.dh = ix->d_hidden; q.dl = ix->d_low; q.dl_pad = ix->dl_pad; q.nq = nx; q.xstride = xstride;
    q.cus = ix->cus; q.in_flight = in_flight; q.mfma = mfma;
    q.mlp_net = ix->knob.mlp_net; q.mlp_slab = ix->knob.mlp_slab; q.mlp_small = ix->knob.mlp_small;
    q.x = x;
    q.w[0] = ix->w1; q.w[1] = ix->w2; q.w[2] = ix->w3;
    q.ws[0] = ix->ws1; q.ws[1] = ix->ws2; q.ws[2] = ix->ws3;
    return q;
}

// MLP over rows x [nx x xstride] (device) -> out [nx x dl_pad] (device); h1/h2 are scratch.
int run_project(gbnns_index* ix, Lane& L, const float* x, uint32_t xstride, uint32_t nx, float* out,
                hipStream_t s, bool in_flight, bool mfma) {
    const ProjShape q = shape_of(ix, x, xstride, nx, in_flight, mfma);
    const ProjRoute r = project_route(q, nullptr);
    ProjPlan& ran = ix->proj_last;   // what the launchers report: the instances this projection ran on
    ran = ProjPlan{};
    const float* bias[3] = {ix->b1, ix->b2, ix->b3};
    if (r.path == ProjPath::Net) {
        NetLaunch n = net_of(q);
        n.out = out; n.form = r.form;
        for (int l = 0; l < 3; ++l) { n.bias[l] = bias[l]; n.img[l] = ix->net_img[n.form][l]; }
        HIP_TRY(launch_mlp_net(n, s, &ran));
        ix->net_form = n.form;
        std::snprintf(ix->acc.project_kernel, sizeof(ix->acc.project_kernel), "mlp_net_kernel");
        return GBNNS_OK;
    }
    if (r.path == ProjPath::MfmaNet) {
        NetLaunch n = net_of(q);
        n.out = out;
        for (int l = 0; l < 3; ++l) n.bias[l] = bias[l];
        if (!ix->net_mfma_ready) {
            int rc0 = ix->net_mfma.ensure(mlp_mfma_net_packed_floats(ix->d, ix->d_hidden, ix->d_low) * 4);
            if (rc0) return rc0;
            HIP_TRY(launch_mlp_mfma_pack(n, ix->net_mfma.as<float>(), s));   // (stream order: before this call's projection; later calls on
            HIP_TRY(hipStreamSynchronize(s));                                  //  other streams find it finished)
            ix->net_mfma_ready = true;
        }
        HIP_TRY(launch_mlp_mfma_net(n, ix->net_mfma.as<float>(), s, &ran));
        std::snprintf(ix->acc.project_kernel, sizeof(ix->acc.project_kernel), "mlp_mfma_net_kernel");
        return GBNNS_OK;
    }
    std::snprintf(ix->acc.project_kernel, sizeof(ix->acc.project_kernel), mfma ? "mlp_layer_mfma_kernel" : "mlp_layer_kernels");
    int rc = L.h1.ensure((size_t)nx * ix->d_hidden * 4);
    if (!rc) rc = L.h2.ensure((size_t)nx * ix->d_hidden * 4);
    if (rc) return rc;
    float* act[3] = {L.h1.as<float>(), L.h2.as<float>(), out};
    bool slab_used = false;
    for (int l = 0; l < 3; ++l) {
        LayerParams p = layer_of(q, l, r.small_footprint, l ? act[l - 1] : nullptr);
        p.bias = bias[l]; p.out = act[l];
        switch (r.layer[l]) {
            case LayerPath::Mfma: HIP_TRY(launch_mlp_layer_mfma(p, s, &ran)); break;
            case LayerPath::Slab: slab_used = true; HIP_TRY(launch_mlp_slab(p, ix->cus, s, 0, &ran)); break;
            case LayerPath::Layer: HIP_TRY(launch_mlp_layer(p, s, &ran)); break;
        }
    }
    if (slab_used) std::snprintf(ix->acc.project_kernel, sizeof(ix->acc.project_kernel), "mlp_slab_kernel");
    return GBNNS_OK;
}

// One dispatch for both stand-alone re-ranks: the kind's parameter struct, filled from the handle, into the kind's launcher.
template <class P>
hipError_t rerank_launch(const gbnns_index* ix, const P& r, hipStream_t s) {
    constexpr bool topk = std::is_same<P, RerankTopkParams>::value;
    const int metric = ix->metric;
    auto of_kind = [&](auto k) {  // (k: an empty parameter struct of the kind)
        static_cast<P&>(k) = r;
        k.db = nullptr; k.dstride = ix->d_pad;
        return k;
    };
    switch (ix->rows) {
        case RowKind::U8: {
            RerankBytesParams b = of_kind(RerankBytesParams{});
            b.db_b = ix->base_as<uint8_t>();
            return topk ? launch_rerank_topk_bytes(b, metric, s) : launch_rerank_bytes(b, metric, s);
        }
        case RowKind::F16: {
            RerankHalfParams h = of_kind(RerankHalfParams{});
            h.db_h = ix->base_as<uint16_t>();
            return topk ? launch_rerank_topk_half(h, metric, s) : launch_rerank_half(h, metric, s);
        }
        case RowKind::F32: break;
    }
    P f = r;
    f.db = ix->base_as<float>(); f.dstride = ix->d_pad;
    if constexpr (topk) return launch_rerank_topk(f, metric, s);
    else return launch_rerank(f, metric, s);
}
template hipError_t rerank_launch<RerankParams>(const gbnns_index*, const RerankParams&, hipStream_t);
template hipError_t rerank_launch<RerankTopkParams>(const gbnns_index*, const RerankTopkParams&, hipStream_t);

int prof_flush(gbnns_index* ix) {
    for (auto& pc : ix->pending) {
        HIP_TRY(hipEventSynchronize(pc.ev[4]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, pc.ev[0], pc.ev[1]));
        ix->acc.project_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, pc.ev[1], pc.ev[2]));
        ix->acc.walk_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, pc.ev[2], pc.ev[3]));
        ix->acc.walk_general_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, pc.ev[3], pc.ev[4]));
        ix->acc.rerank_ms += ms;
        HIP_TRY(hipEventElapsedTime(&ms, pc.ev[0], pc.ev[4]));
        ix->acc.total_ms += ms;
        ix->acc.calls += 1;
        ix->acc.queries += pc.queries;
        for (int i = 0; i < 5; ++i) (void)hipEventDestroy(pc.ev[i]);
    }
    ix->pending.clear();
    return GBNNS_OK;
}

}  // namespace gbnns_api

extern "C" {

// Diagnostic (not in gbnns.h): copies the 32 stamp/histogram sums of a GBNNS_STAMPS build and clears them.
int gbnns_debug_read_stamps(gbnns_index* ix, unsigned long long* out32) {
    if (!ix || !out32) return fail(GBNNS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out32, ix->lanes[0].ctrl.as<uint32_t>() + 8, 256, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemset(ix->lanes[0].ctrl.as<uint32_t>() + 8, 0, 256));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return GBNNS_OK;
}

// Diagnostic (not in gbnns.h): one batch merge of the register-list walk kernels on host-supplied keys.
// entries: sorted u64 keys [size]; surv: 64 keys, ~0 = no survivor in that lane; out: 64*regs keys;
// out_info: {new size, merged (0 = boundary tie, list untouched), new worst}.
int gbnns_debug_merge(int regs, const unsigned long long* entries, int size, const unsigned long long* surv, int ef,
                      unsigned long long* out, int* out_info) {
    if (!(regs == 1 || regs == 2 || regs == 4) || size < 1 || size > ef || ef > 64 * regs)
        return fail(GBNNS_ERR_INVALID, "bad debug_merge arguments");
    unsigned long long *d_e = nullptr, *d_s = nullptr, *d_o = nullptr;
    int* d_i = nullptr;
    HIP_TRY(hipMalloc(&d_e, 256 * 8));
    HIP_TRY(hipMalloc(&d_s, 64 * 8));
    HIP_TRY(hipMalloc(&d_o, 256 * 8));
    HIP_TRY(hipMalloc(&d_i, 16));
    HIP_TRY(hipMemcpy(d_e, entries, (size_t)size * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_s, surv, 64 * 8, hipMemcpyHostToDevice));
    HIP_TRY(launch_debug_merge(regs, reinterpret_cast<const uint64_t*>(d_e), size, reinterpret_cast<const uint64_t*>(d_s), ef,
                               reinterpret_cast<uint64_t*>(d_o), d_i, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, d_o, (size_t)64 * regs * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_info, d_i, 12, hipMemcpyDeviceToHost));
    (void)hipFree(d_e); (void)hipFree(d_s); (void)hipFree(d_o); (void)hipFree(d_i);
    return GBNNS_OK;
}

int gbnns_debug_knob(const char* name, int value) {
    if (!name) return fail(GBNNS_ERR_INVALID, "gbnns_debug_knob: null name");
    if (knob_default_set(name, value)) return GBNNS_OK;  // a handle knob: the default of the handles created from now on
    if (!std::strcmp(name, "knn_chunk")) g_knob_knn_chunk.store(std::max(64, value & ~63), std::memory_order_relaxed);
    else if (!std::strcmp(name, "knn_pool_min_k")) g_knob_knn_pool_min_k.store(std::max(1, value), std::memory_order_relaxed);
    else if (!std::strcmp(name, "knn_filter")) g_knob_knn_filter.store(value, std::memory_order_relaxed);
    else if (!std::strcmp(name, "knn_slab")) g_knob_knn_slab.store(value > 0 ? std::max(128, value & ~127) : 0, std::memory_order_relaxed);
    else return fail(GBNNS_ERR_INVALID, "gbnns_debug_knob: unknown knob '%s'", name);
    return GBNNS_OK;
}

int gbnns_debug_net_lds(uint32_t d, uint32_t d_hidden, uint32_t d_low, int form, int a, uint64_t* lds_bytes, int* admitted) {
    if (!lds_bytes || !admitted) return fail(GBNNS_ERR_INVALID, "gbnns_debug_net_lds: null output");
    if (!d || !d_hidden || !d_low || a < 2 || a > 5 || (form != kNetWholeCu && form != kNetHalfCu))
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_net_lds: no such net, form or strip");
    NetLaunch n{};
    n.din[0] = d; n.din[1] = n.din[2] = d_hidden;
    n.dout[0] = n.dout[1] = d_hidden; n.dout[2] = d_low;
    *lds_bytes = mlp_net_lds_bytes(n, form, a);
    *admitted = mlp_net_lds_bytes(n, form, 4) <= (form == kNetHalfCu ? 80u : 160u) * 1024u;
    return GBNNS_OK;
}

static void plan_names(const ProjPlan& plan, char* names, uint32_t names_bytes) {
    std::string all;
    for (int i = 0; i < plan.count; ++i) {
        char one[64];
        proj_instance_name(plan.inst[i], one, sizeof one);
        if (i) all += '\n';
        all += one;
    }
    std::snprintf(names, names_bytes, "%s", all.c_str());
}

int gbnns_debug_project_plan(uint32_t d, uint32_t d_hidden, uint32_t d_low, uint64_t n_q, int cus, int in_flight, int mfma, int mlp_net,
                             int mlp_slab, int mlp_small, char* names, uint32_t names_bytes) {
    if (!names || !names_bytes) return fail(GBNNS_ERR_INVALID, "gbnns_debug_project_plan: no room for the names");
    if (!d || !d_hidden || !d_low || !n_q || n_q >= (1ull << 31) || cus < 1)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_project_plan: no such net, batch or device");
    if (mlp_net < 0 || mlp_net > 3 || mlp_slab < 0 || mlp_slab > 2 || mlp_small < 0)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_project_plan: a knob value outside its range");
    gbnns_api::ProjShape q{};
    q.d = d; q.dh = d_hidden; q.dl = d_low; q.dl_pad = round_up(d_low, 4); q.nq = (uint32_t)n_q; q.xstride = d;
    q.cus = cus; q.in_flight = in_flight != 0; q.mfma = mfma != 0;
    q.mlp_net = mlp_net; q.mlp_slab = mlp_slab; q.mlp_small = mlp_small;
    q.ws[0] = round_up(d, 16); q.ws[1] = q.ws[2] = round_up(d_hidden, 16);   // (the handle's repacked rows; x and w stay null: aligned)
    ProjPlan plan;
    (void)gbnns_api::project_route(q, &plan);
    plan_names(plan, names, names_bytes);
    return GBNNS_OK;
}

int gbnns_index_project_last(gbnns_index* ix, char* names, uint32_t names_bytes) {
    if (!ix || !names || !names_bytes) return fail(GBNNS_ERR_INVALID, "gbnns_index_project_last: null argument");
    plan_names(ix->proj_last, names, names_bytes);
    return GBNNS_OK;
}

// The locality order of host queries [n_q x qstride] on their first `bits` coordinates (clamped to 10 .. 16): launch_query_order alone, on
// the current device, its histogram and order buffers this call's own.  The launcher's refusal (dim < bits after clamping) is the call's.
int gbnns_debug_query_order(const float* queries, uint32_t qstride, uint32_t dim, uint64_t n_q, int bits, uint32_t* out_order) {
    if (!queries || !out_order) return fail(GBNNS_ERR_INVALID, "gbnns_debug_query_order: null argument");
    if (!dim || qstride < dim || !n_q || n_q >= (1ull << 31) || bits < 0)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_query_order: no such batch");
    const size_t qbytes = (size_t)n_q * qstride * 4, obytes = (size_t)n_q * 4;
    ScopedDevBuf q, hist, order;
    int rc;
    // (order: room for 2 n_q entries -- a scatter whose cursors start too high, by up to a bucket's size, still writes inside the buffer;
    // all ones first: a slot the scatter leaves out is no valid query)
    if ((rc = q.ensure(qbytes)) || (rc = hist.ensure((size_t)4 << 16)) || (rc = order.ensure(2 * obytes))) return rc;
    if ((rc = h2d_staged(q.p, queries, qbytes))) return rc;
    HIP_TRY(hipMemset(order.p, 0xFF, 2 * obytes));
    HIP_TRY(launch_query_order(q.as<float>(), qstride, dim, (uint32_t)n_q, (uint32_t)bits, hist.as<uint32_t>(), order.as<uint32_t>(), nullptr));
    return d2h_staged(out_order, order.p, obytes, nullptr);
}

// The permutation the handle's last ordered search call walked its batch in (knob "order_last": whether the very last call was one), read
// from that call's lane once everything enqueued on the device has completed.  capacity: entries out_order holds; *out_n: that call's
// queries -- set also where out_order is NULL or too small (GBNNS_ERR_INVALID, nothing copied), so a caller can ask for the size first.
int gbnns_index_order_last(gbnns_index* ix, uint32_t* out_order, uint64_t capacity, uint64_t* out_n) {
    if (!ix || !out_n) return fail(GBNNS_ERR_INVALID, "gbnns_index_order_last: null argument");
    *out_n = 0;
    if (ix->order_perm_lane < 0) return fail(GBNNS_ERR_INVALID, "gbnns_index_order_last: no call of this handle was walked in locality order");
    *out_n = ix->order_perm_n;
    if (!out_order || capacity < ix->order_perm_n)
        return fail(GBNNS_ERR_INVALID, "gbnns_index_order_last: room for %llu entries, the order has %u", (unsigned long long)(out_order ? capacity : 0),
                    ix->order_perm_n);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // (the call may have run on a lane's own stream, its join still owed)
    return d2h_staged(out_order, ix->lanes[ix->order_perm_lane].order.p, (size_t)ix->order_perm_n * 4, nullptr);
}

// Diagnostic (not in gbnns.h; host only, no device): the staged-order image of one layer (kernels.h pack_net_image) for host weights
// w [dout x wstride], b neurons per lane group (8 hidden; last layer: *b3_of_d_low says which), go neuron groups (2 whole-CU, 4 half-CU).
// out == NULL: only the sizes.  geom: {ck, ldw, rows, buf, nch, slices, interleaved, floats of the image}.
int gbnns_debug_net_image(const float* w, uint32_t wstride, uint32_t din, uint32_t dout, uint32_t b, uint32_t go, float* out,
                          uint64_t out_floats, uint64_t* geom8, uint32_t* b3_of_dout) {
    if (!geom8 || !din || !dout || !(b == 2 || b == 4 || b == 8) || !(go == 2 || go == 4) || wstride < round_up(din, 16))
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_net_image: no such layer or form");
    const NetImageGeom g = net_image_geom(din, dout, b, go);
    const uint64_t floats = net_image_floats(din, dout, b, go);
    const uint64_t v[8] = {g.ck, g.ldw, g.rows, g.buf, g.nch, g.slices, g.interleaved ? 1u : 0u, floats};
    std::memcpy(geom8, v, sizeof v);
    if (b3_of_dout) *b3_of_dout = net_image_b3(dout);
    if (!out) return GBNNS_OK;
    if (!w || out_floats < floats) return fail(GBNNS_ERR_INVALID, "gbnns_debug_net_image: output of %llu floats needed", (unsigned long long)floats);
    pack_net_image(w, wstride, din, dout, b, go, out);
    return GBNNS_OK;
}

// The six plan diagnostics below: one validation, the walked shape filled by the function search_core.cpp fills its own with (set_walk_shape,
// call_plan.h), one plan_walk.  `f`: the handle's and the call's facts as the endpoint states them; `w`: the decisions it was given (late /
// speculative rows, rr_reserve, bytes_dim); coop: asked for, taken where the shape has an instance.  general_lds: what *lds_bytes holds when
// the general kernel takes the whole batch (0: the plan's figure).
static int debug_plan(const char* fn, CallFacts f, WalkParams w, int force_wide, int coop, int pass, uint64_t general_lds, char* name, uint32_t name_bytes,
                      uint64_t* lds_bytes, int* fused) {
    if (!name || name_bytes == 0 || !(lds_bytes || fused)) return fail(GBNNS_ERR_INVALID, "%s: null output", fn);
    if ((f.metric != GBNNS_METRIC_L2 && f.metric != GBNNS_METRIC_NEG_DOT) || f.dim == 0 || f.dstride != row_pad(f.dim, f.walked) || f.n == 0 ||
        f.n > 0xFFFFFFFFull || f.ell_stride == 0 || f.ell_stride % 16 || f.aux_stride % 16 || f.ef < 1 || f.n_entries > 4096 || pass < 0 || pass > 2)
        return fail(GBNNS_ERR_INVALID, "%s: not the shape of an index or a search", fn);
    f.flags = force_wide ? GBNNS_FLAG_WIDE_INDEX : 0u;
    f.knob.hot = 1;
    set_walk_shape(w, f);
    const WalkPass wp = pass == 1 ? WalkPass::Bitmap : (pass == 2 ? WalkPass::Retry : WalkPass::First);
    w.coop = coop && wp == WalkPass::First && plan_walk(w, f.metric, wp).coop_serves;
    const WalkPlan plan = plan_walk(w, f.metric, wp);
    const char* planned = plan.general_only ? "walk_general_kernel" : walk_plan_name(plan);
    if (!planned) return fail(GBNNS_ERR_INTERNAL, "%s: no kernel instance for the plan", fn);
    std::snprintf(name, name_bytes, "%s", planned);
    if (lds_bytes) *lds_bytes = (plan.general_only && general_lds) ? general_lds : plan.lds_fixed;
    if (fused) *fused = (!plan.general_only && (plan.inst.flags & kRrBytes)) ? 1 : 0;
    return GBNNS_OK;
}

static CallFacts debug_facts(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries) {
    CallFacts f{};
    f.metric = metric; f.dim = dim; f.dstride = dstride; f.n = n; f.ell_stride = ell_stride; f.aux_stride = aux_stride; f.ef = ef; f.n_entries = n_entries;
    return f;
}

int gbnns_debug_walk_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                          uint32_t n_entries, int force_wide, int coop, int late_rows, int spec_rows, int pass, uint32_t rr_reserve,
                          char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    if (!lds_bytes) return fail(GBNNS_ERR_INVALID, "gbnns_debug_walk_plan: null output");
    WalkParams w{};
    w.late_rows = late_rows != 0; w.spec_rows = spec_rows != 0; w.rr_reserve = rr_reserve;
    return debug_plan("gbnns_debug_walk_plan", debug_facts(metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries), w, force_wide, coop, pass, 0, name,
                      name_bytes, lds_bytes, nullptr);
}

int gbnns_debug_byte_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                          uint32_t n_entries, int force_wide, int coop, int late_rows, int spec_rows, int pass, uint32_t rr_reserve,
                          char* name, uint32_t name_bytes, int* fused) {
    if (!fused) return fail(GBNNS_ERR_INVALID, "gbnns_debug_byte_plan: null output");
    WalkParams w{};
    w.late_rows = late_rows != 0; w.spec_rows = spec_rows != 0; w.rr_reserve = rr_reserve;
    w.bytes_dim = metric == GBNNS_METRIC_L2 ? 16u : 0u;  // (an original dimension the chunk-pair re-rank serves: CallPlan::bytes_dim of such a handle)
    return debug_plan("gbnns_debug_byte_plan", debug_facts(metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries), w, force_wide, coop, pass, 0, name,
                      name_bytes, nullptr, fused);
}

int gbnns_debug_rerank_plan(int metric, uint32_t d, int bytes, char* name, uint32_t name_bytes, int* deep, int* fused) {
    if (!name || name_bytes == 0 || !deep || !fused) return fail(GBNNS_ERR_INVALID, "gbnns_debug_rerank_plan: null output");
    if ((metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) || d == 0)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_rerank_plan: not the metric or the dimension of an index");
    const RerankPlan plan = rerank_plan(metric, d, bytes != 0);
    if (plan.form == RerankForm::ChunkPairs) std::snprintf(name, name_bytes, "rerank_bytes_pair_kernel");
    else std::snprintf(name, name_bytes, "%s<%d>", bytes ? "rerank_bytes_kernel" : (plan.form == RerankForm::Pairs ? "rerank_pair_kernel" : "rerank_kernel"), metric);
    *deep = plan.deep;
    *fused = plan.fuses ? 1 : 0;
    return GBNNS_OK;
}

int gbnns_debug_half_base_plan(int metric, uint32_t d, char* name, uint32_t name_bytes, int* deep, int* fused) {
    if (!name || name_bytes == 0 || !deep || !fused) return fail(GBNNS_ERR_INVALID, "gbnns_debug_half_base_plan: null output");
    if ((metric != GBNNS_METRIC_L2 && metric != GBNNS_METRIC_NEG_DOT) || d == 0)
        return fail(GBNNS_ERR_INVALID, "gbnns_debug_half_base_plan: not the metric or the dimension of an index");
    const RerankPlan plan = rerank_half_plan(metric, d);
    if (plan.form == RerankForm::HalfChunkPairs) std::snprintf(name, name_bytes, "rerank_half_pair_kernel");
    else std::snprintf(name, name_bytes, "rerank_half_kernel<%d>", metric);
    *deep = plan.deep;
    *fused = plan.fuses ? 1 : 0;
    return GBNNS_OK;
}

// (a flagged PLAIN call on a byte handle: rows of round_up(dim, 16) bytes; the general kernel: the staged query alone)
static int debug_byte_walk_plan(const char* fn, bool byte_queries, int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef,
                                uint32_t n_entries, int force_wide, int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    if (!lds_bytes) return fail(GBNNS_ERR_INVALID, "%s: null output", fn);
    CallFacts f = debug_facts(metric, dim, row_pad(dim, RowKind::U8), n, ell_stride, aux_stride, ef, n_entries);
    f.tagged = tagged != 0; f.rows = f.walked = RowKind::U8;
    f.byte_queries = byte_queries; f.knob.byte_query_int = 7;  // (... and whether the call brought byte queries; every beam class: knob "byte_query_int" = 7)
    return debug_plan(fn, f, WalkParams{}, force_wide, 0, 0, (uint64_t)f.dstride * 4u, name, name_bytes, lds_bytes, nullptr);
}

int gbnns_debug_byte_walk_plan(int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries, int force_wide,
                               int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    return debug_byte_walk_plan("gbnns_debug_byte_walk_plan", false, metric, dim, n, ell_stride, aux_stride, ef, n_entries, force_wide, tagged, name, name_bytes, lds_bytes);
}

// (a flagged PLAIN call on a half-base handle: rows of round_up(dim, 8) halves, knob "half_walk_fast" = 2: every instance the unit has; the general kernel: the staged query alone)
int gbnns_debug_half_walk_plan(int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries, int force_wide,
                               int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    if (!lds_bytes) return fail(GBNNS_ERR_INVALID, "gbnns_debug_half_walk_plan: null output");
    CallFacts f = debug_facts(metric, dim, row_pad(dim, RowKind::F16), n, ell_stride, aux_stride, ef, n_entries);
    f.tagged = tagged != 0; f.rows = f.walked = RowKind::F16; f.knob.half_walk_fast = 2;
    return debug_plan("gbnns_debug_half_walk_plan", f, WalkParams{}, force_wide, 0, 0, (uint64_t)f.dstride * 4u, name, name_bytes, lds_bytes, nullptr);
}

int gbnns_debug_byte_query_plan(int metric, uint32_t dim, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries, int force_wide,
                                int tagged, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    return debug_byte_walk_plan("gbnns_debug_byte_query_plan", true, metric, dim, n, ell_stride, aux_stride, ef, n_entries, force_wide, tagged, name, name_bytes, lds_bytes);
}

static int debug_tag_plan(const char* fn, bool bridged, int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries,
                          int force_wide, uint32_t rr_reserve, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    if (!lds_bytes) return fail(GBNNS_ERR_INVALID, "%s: null output", fn);
    CallFacts f = debug_facts(metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries);
    f.tagged = true; f.bridged = bridged;
    WalkParams w{};
    w.rr_reserve = rr_reserve;
    return debug_plan(fn, f, w, force_wide, 0, 0, 0, name, name_bytes, lds_bytes, nullptr);
}

int gbnns_debug_tag_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries,
                         int force_wide, uint32_t rr_reserve, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    return debug_tag_plan("gbnns_debug_tag_plan", false, metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries, force_wide, rr_reserve, name, name_bytes, lds_bytes);
}

int gbnns_debug_bridge_plan(int metric, uint32_t dim, uint32_t dstride, uint64_t n, uint32_t ell_stride, uint32_t aux_stride, int ef, uint32_t n_entries,
                            int force_wide, uint32_t rr_reserve, char* name, uint32_t name_bytes, uint64_t* lds_bytes) {
    return debug_tag_plan("gbnns_debug_bridge_plan", true, metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries, force_wide, rr_reserve, name, name_bytes, lds_bytes);
}

// ---- gbnns_search_tagged: the rows' tag words -------------------------------------------------------------------------------------------

int gbnns_index_set_tags(gbnns_index* ix, const uint32_t* tags, uint64_t first, uint64_t count, int mem_kind, void* stream) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    if (mem_kind != GBNNS_MEM_HOST && mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", mem_kind);
    if (!tags && count) return fail(GBNNS_ERR_INVALID, "gbnns_index_set_tags: null tags");
    if (first > ix->n || count > ix->n - first)
        return fail(GBNNS_ERR_INVALID, "gbnns_index_set_tags: rows [%llu, %llu) outside n = %llu", (unsigned long long)first,
                    (unsigned long long)(first + count), (unsigned long long)ix->n);
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!tags) {  // drop the table: nothing in flight may still read it
        HIP_TRY(hipDeviceSynchronize());
        ix->tags.release();
        return GBNNS_OK;
    }
    // (the table is ordered like the rest of the handle's state: by stream order, a call on another stream first waits for the work in flight)
    if (int rc = enter_stream(ix, s)) return rc;
    if (!ix->tags.p) {
        const size_t bytes = (size_t)ix->n * 4;  // exactly sized
        const hipError_t e = hipMalloc(&ix->tags.p, bytes);
        if (e != hipSuccess) {
            ix->tags.p = nullptr;
            return fail(GBNNS_ERR_OOM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        }
        ix->tags.bytes = bytes;
        HIP_TRY(launch_fill_u32(ix->tags.as<uint32_t>(), 0xFFFFFFFFu, (size_t)ix->n, s));
    }
    uint32_t* dst = ix->tags.as<uint32_t>() + first;
    if (mem_kind == GBNNS_MEM_DEVICE) {
        if (count) HIP_TRY(hipMemcpyAsync(dst, tags, (size_t)count * 4, hipMemcpyDeviceToDevice, s));
        return GBNNS_OK;
    }
    if (int rc = host_copy_in(ix->lanes[0], dst, tags, (size_t)count * 4, s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    ix->in_flight = false;
    return GBNNS_OK;
}

// ---- GBNNS_FLAG_HALF_ROWS: the rounded table ---------------------------------------------------------------------------------------------

namespace {
// float32 -> binary16, round to nearest, ties to even; subnormals and the sign of zero kept.  false: not finite, or rounds out of range.
bool float_to_half_bits(float f, uint16_t& h) {
    uint32_t x;
    std::memcpy(&x, &f, 4);
    const uint32_t sign = (x >> 16) & 0x8000u, ax = x & 0x7FFFFFFFu;
    if (ax >= 0x477FF000u) return false;  // |f| >= 65 520 = the midpoint between 65 504 and 2^16 (ties to even: up), infinities, NaNs
    const uint32_t e = ax >> 23;
    uint32_t q, rem, halfway;
    if (e < 113u) {  // |f| < 2^-14: a binary16 subnormal (units of 2^-24) or zero
        const uint32_t m = e ? ((ax & 0x7FFFFFu) | 0x800000u) : 0u, shift = 126u - e;  // |f| = m * 2^(e - 150) = m * 2^-shift units
        if (shift > 25u || m == 0u) { h = (uint16_t)sign; return true; }           // (m < 2^24: below half a unit)
        q = m >> shift; rem = m & ((1u << shift) - 1u); halfway = 1u << (shift - 1u);
    } else {
        q = ((e - 112u) << 10) | ((ax & 0x7FFFFFu) >> 13); rem = ax & 0x1FFFu; halfway = 0x1000u;
    }
    if (rem > halfway || (rem == halfway && (q & 1u))) q += 1u;  // (a carry out of the mantissa is the next exponent's first value)
    h = (uint16_t)(sign | q);
    return true;
}
float half_bits_to_float(uint16_t h) {
    const uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
    const float v = e ? std::ldexp((float)(1024u + m), (int)e - 25) : std::ldexp((float)m, -24);
    return (h & 0x8000u) ? -v : v;
}
}  // namespace

int gbnns_round_to_half(const float* in, uint64_t count, uint16_t* out_bits, float* out_widened) {
    if (!in && count) return fail(GBNNS_ERR_INVALID, "gbnns_round_to_half: null input");
    for (uint64_t i = 0; i < count; ++i) {
        uint16_t h;
        if (!float_to_half_bits(in[i], h))
            return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_round_to_half: value %llu (%g) is not finite or rounds out of the binary16 range",
                        (unsigned long long)i, (double)in[i]);
        if (out_bits) out_bits[i] = h;
        if (out_widened) out_widened[i] = half_bits_to_float(h);
    }
    return GBNNS_OK;
}

int gbnns_index_enable_half_rows(gbnns_index* ix) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null argument");
    if (!ix->db_low) return fail(GBNNS_ERR_INVALID, "gbnns_index_enable_half_rows: the index has no db_low");
    if (ix->half_ready) return GBNNS_OK;
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipDeviceSynchronize());  // (a borrowed db_low may have been written on any stream)
    const uint32_t hstride = round_up(ix->d_low, 8);
    // exactly sized (DevBuf::ensure adds slack for buffers that grow): 0.5 + 1 times the low-dimensional table
    DevBuf h, r, flag;
    auto alloc = [](DevBuf& b, size_t bytes) -> int {
        const hipError_t e = hipMalloc(&b.p, bytes);
        if (e != hipSuccess) {
            b.p = nullptr;
            return fail(GBNNS_ERR_OOM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        }
        b.bytes = bytes;
        return GBNNS_OK;
    };
    int rc = alloc(h, (size_t)ix->n * hstride * 2);
    if (!rc) rc = alloc(r, (size_t)ix->n * ix->dl_pad * 4);
    if (!rc) rc = alloc(flag, 4);
    uint32_t bad = 0xFFFFFFFFu;
    if (!rc) {
        hipError_t e = hipMemcpy(flag.p, &bad, 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e == hipSuccess)
            e = launch_half_rows_convert(ix->db_low, ix->dl_pad, ix->d_low, ix->n, h.as<uint16_t>(), hstride, r.as<float>(), ix->dl_pad, flag.as<uint32_t>(), nullptr);
        if (e == hipSuccess) e = hipMemcpy(&bad, flag.p, 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) rc = fail(GBNNS_ERR_HIP, "gbnns_index_enable_half_rows: %s", hipGetErrorString(e));
    }
    if (!rc && bad != 0xFFFFFFFFu)
        rc = fail(GBNNS_ERR_UNSUPPORTED, "gbnns_index_enable_half_rows: row %u of db_low holds a value that is not finite or rounds out of the binary16 range", bad);
    flag.release();
    if (rc) {  // the handle stays as it was
        h.release();
        r.release();
        return rc;
    }
    ix->low_half = h;
    ix->low_r = r;
    ix->half_ready = true;
    return GBNNS_OK;
}

int gbnns_index_low_rows(gbnns_index* ix, float* out, int mem_kind, void* stream) {
    if (!ix || !out) return fail(GBNNS_ERR_INVALID, "null argument");
    if (mem_kind != GBNNS_MEM_HOST && mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", mem_kind);
    if (!ix->half_ready) return fail(GBNNS_ERR_INVALID, "gbnns_index_low_rows: gbnns_index_enable_half_rows has not been called");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t spitch = (size_t)ix->dl_pad * 4, width = (size_t)ix->d_low * 4;
    if (mem_kind == GBNNS_MEM_DEVICE) {
        HIP_TRY(hipMemcpy2DAsync(out, width, ix->low_r.p, spitch, width, ix->n, hipMemcpyDeviceToDevice, s));
        return GBNNS_OK;
    }
    if (int rc = enter_stream(ix, s)) return rc;  // (lane 0's staging buffer is ordered by stream order, like the rest of the workspace)
    if (int rc = host_copy_out(ix->lanes[0], out, ix->low_r.p, spitch, width, ix->n, s)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    ix->in_flight = false;
    return GBNNS_OK;
}

int gbnns_index_knob_get(gbnns_index* ix, const char* name, int* out) {
    if (!name || !out) return fail(GBNNS_ERR_INVALID, "gbnns_index_knob_get: null argument");
    if (!ix) {  // no handle, no device: the process-wide default a new handle would start from (the two locality-order knobs)
        const Knobs d = knob_defaults();
        if (!std::strcmp(name, "order_min")) { *out = d.order_min; return GBNNS_OK; }
        if (!std::strcmp(name, "order_bits")) { *out = d.order_bits; return GBNNS_OK; }
        return fail(GBNNS_ERR_INVALID, "gbnns_index_knob_get: null argument");
    }
    const Knobs& k = ix->knob;
    const struct { const char* n; int v; } all[] = {
        {"quotient", k.quotient}, {"vs_disp", k.vs_disp}, {"max_waves", k.max_waves}, {"spec_min_nq", k.spec_min_nq},
        {"spec_any_form", k.spec_any_form}, {"mlp_small", k.mlp_small}, {"mlp_net", k.mlp_net}, {"mlp_slab", k.mlp_slab},
        {"late_rows", k.late_rows}, {"spec_tail", k.spec_tail}, {"coop", k.coop}, {"hot", k.hot}, {"byte_query_int", k.byte_query_int}, {"half_walk_fast", k.half_walk_fast}, {"mlp_net_form", ix->net_form}, {"cus", ix->cus},
        {"gather_budget", k.gather_budget}, {"gather_timing", k.gather_timing}, {"gather_census_us", ix->gather_us[0]}, {"gather_fill_us", ix->gather_us[1]},
        {"gather_scan_us", ix->gather_us[2]}, {"gather_rounds", ix->gather_rounds},
        {"order_min", k.order_min}, {"order_bits", k.order_bits}, {"order_last", (int)ix->order_last}};
    for (const auto& e : all)
        if (!std::strcmp(name, e.n)) { *out = e.v; return GBNNS_OK; }
    return fail(GBNNS_ERR_INVALID, "gbnns_index_knob_get: unknown handle knob '%s'", name);
}

int gbnns_index_knob(gbnns_index* ix, const char* name, int value) {
    if (!ix || !name) return fail(GBNNS_ERR_INVALID, "gbnns_index_knob: null argument");
    if (!knob_set(ix->knob, name, value)) return fail(GBNNS_ERR_INVALID, "gbnns_index_knob: unknown handle knob '%s'", name);
    return GBNNS_OK;
}

int gbnns_profile_enable(gbnns_index* ix, int on) {
    if (!ix) return fail(GBNNS_ERR_INVALID, "null index");
    ix->profiling = on != 0;
    return GBNNS_OK;
}

int gbnns_profile_read(gbnns_index* ix, gbnns_profile* out, int reset) {
    if (!ix || !out) return fail(GBNNS_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(ix->device));
    int rc = prof_flush(ix);
    if (rc) return rc;
    uint32_t total = 0;  // ctrl[5]: queries the general kernel has processed since the last reset
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(&total, ix->lanes[0].ctrl.as<uint32_t>() + 5, 4, hipMemcpyDeviceToHost));
    ix->acc.general_queries = total;
    if (ix->prof_ctrl_pending) {  // hand-over counts of the last profiled call (copied behind its general kernel; the device is idle now)
        ix->prof_ctrl_pending = false;
        // (a first pass that appended to list B itself -- no retry launch -- handed all of it on)
        ix->acc.retry_queries = ix->prof_ctrl[ix->prof_ctrl_direct ? 3 : 0];
        ix->acc.retry_general_queries = ix->prof_ctrl[3];
    }
    ix->acc.struct_size = sizeof(gbnns_profile);
    // out->struct_size on entry = the caller's sizeof(gbnns_profile): a caller built against an older header (the struct grew from 160 to
    // 192 bytes in round 5, to 304 with the retry pass's name and counts) gets the prefix it knows and nothing written past it; 0 (callers that never set it) = the 160-byte round-4 layout
    {
        const size_t theirs = out->struct_size ? out->struct_size : 160u;
        const size_t take = std::min(theirs, sizeof(gbnns_profile));
        if (take < 8) return fail(GBNNS_ERR_INVALID, "gbnns_profile.struct_size %zu too small", theirs);
        std::memcpy(out, &ix->acc, take);
        out->struct_size = (uint32_t)take;
    }
    if (reset) {
        ix->acc = gbnns_profile{};
        HIP_TRY(hipMemset(ix->lanes[0].ctrl.as<uint32_t>() + 5, 0, 4));
        HIP_TRY(hipStreamSynchronize(nullptr));  // callers' streams need not order themselves after the null stream
    }
    return GBNNS_OK;
}

int gbnns_project(gbnns_index* ix, const float* x, uint64_t n_x, float* out, int mem_kind,
                  void* stream) {
    if (!ix || !x || !out) return fail(GBNNS_ERR_INVALID, "null argument");
    if (!ix->has_net) return fail(GBNNS_ERR_INVALID, "index has no net");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint64_t chunk = 1u << 16;
    int rc = enter_stream(ix, s);
    if (rc) return rc;
    Lane& L = ix->lanes[0];
    rc = L.q_low.ensure((size_t)std::min<uint64_t>(chunk, n_x) * ix->dl_pad * 4);
    if (rc) return rc;
    if (mem_kind == GBNNS_MEM_HOST) {
        rc = L.q_in.ensure((size_t)std::min<uint64_t>(chunk, n_x) * ix->d * 4);
        if (rc) return rc;
    }
    for (uint64_t b = 0; b < n_x; b += chunk) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(chunk, n_x - b);
        const float* xin = x + b * ix->d;
        if (mem_kind == GBNNS_MEM_HOST) {
            if ((rc = host_copy_in(L, L.q_in.p, xin, (size_t)m * ix->d * 4, s))) return rc;
            xin = L.q_in.as<float>();
        }
        float* dst = L.q_low.as<float>();
        const bool direct = mem_kind == GBNNS_MEM_DEVICE && ix->dl_pad == ix->d_low;
        if (direct) dst = out + b * ix->d_low;
        rc = run_project(ix, L, xin, ix->d, m, dst, s);
        if (rc) return rc;
        if (mem_kind == GBNNS_MEM_HOST) {
            if ((rc = host_copy_out(L, out + b * ix->d_low, dst, (size_t)ix->dl_pad * 4, (size_t)ix->d_low * 4, m, s))) return rc;
        } else if (!direct) {
            HIP_TRY(hipMemcpy2DAsync(out + b * ix->d_low, (size_t)ix->d_low * 4, dst, (size_t)ix->dl_pad * 4,
                                     (size_t)ix->d_low * 4, m, hipMemcpyDeviceToDevice, s));
        }
        if (mem_kind == GBNNS_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    }
    return GBNNS_OK;
}

int gbnns_rerank(gbnns_index* ix, const float* queries, uint64_t n_q, const uint32_t* cand,
                 uint32_t cand_stride, const int32_t* count, uint32_t* out_ids, int mem_kind,
                 void* stream) {
    if (!ix || !queries || !cand || !out_ids) return fail(GBNNS_ERR_INVALID, "null argument");
    if (n_q == 0) return GBNNS_OK;
    if (cand_stride == 0 || n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "bad sizes");
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t nq = (uint32_t)n_q;
    const bool host = mem_kind == GBNNS_MEM_HOST;
    int rc;
    if ((rc = enter_stream(ix, s))) return rc;
    Lane& L = ix->lanes[0];
    RerankParams r{};
    r.dstride = ix->d_pad; r.dim = ix->d; r.qstride = ix->d; r.cand_stride = cand_stride;  // (r.db: rerank_launch, by the handle's row kind)
    r.nq = nq; r.n = (uint32_t)ix->n;
    if ((rc = L.cnt.ensure((size_t)nq * 4))) return rc;
    int32_t* cnt_dev = L.cnt.as<int32_t>();
    if (host) {
        if ((rc = L.q_in.ensure((size_t)nq * ix->d * 4))) return rc;
        if ((rc = L.cand.ensure((size_t)nq * cand_stride * 4))) return rc;
        if ((rc = L.out.ensure((size_t)nq * 4))) return rc;
        for (uint64_t i = 0; i < n_q; ++i) {
            const uint32_t c = count ? (uint32_t)std::max(count[i], 0) : cand_stride;
            if (c > cand_stride) return fail(GBNNS_ERR_INVALID, "count[%llu] > stride", (unsigned long long)i);
            for (uint32_t j = 0; j < c; ++j)
                if (cand[i * cand_stride + j] >= ix->n)
                    return fail(GBNNS_ERR_INVALID, "candidate id %u >= n", cand[i * cand_stride + j]);
        }
        if ((rc = host_copy_in(L, L.q_in.p, queries, (size_t)nq * ix->d * 4, s))) return rc;
        if ((rc = host_copy_in(L, L.cand.p, cand, (size_t)nq * cand_stride * 4, s))) return rc;
        if (count && (rc = host_copy_in(L, cnt_dev, count, (size_t)nq * 4, s))) return rc;
        r.q = L.q_in.as<float>(); r.cand = L.cand.as<uint32_t>(); r.out = L.out.as<uint32_t>();
    } else {
        r.q = queries; r.cand = cand; r.out = out_ids;
        if (count) cnt_dev = const_cast<int32_t*>(count);
    }
    if (!count) HIP_TRY(launch_fill_u32(reinterpret_cast<uint32_t*>(cnt_dev), cand_stride, nq, s));
    r.count = cnt_dev;
    HIP_TRY(rerank_launch(ix, r, s));
    if (host) {
        if ((rc = host_copy_out(L, out_ids, r.out, (size_t)nq * 4, (size_t)nq * 4, 1, s))) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        ix->in_flight = false;
    }
    return GBNNS_OK;
}

int gbnns_rerank_topk(gbnns_index* ix, const float* queries, uint64_t n_q, const uint32_t* cand, uint32_t cand_stride,
                      const int32_t* count, int k, uint32_t* out_ids, float* out_dist, int mem_kind, void* stream) {
    // (what needs neither the handle nor a device first, then what needs no device)
    if (!queries || !cand || !out_ids) return fail(GBNNS_ERR_INVALID, "null argument");
    if (cand_stride == 0 || n_q >= (1ull << 31)) return fail(GBNNS_ERR_INVALID, "bad sizes");
    if (k < 1 || (uint32_t)k > cand_stride) return fail(GBNNS_ERR_INVALID, "k = %d outside 1 .. cand_stride = %u", k, cand_stride);
    if (mem_kind != GBNNS_MEM_HOST && mem_kind != GBNNS_MEM_DEVICE) return fail(GBNNS_ERR_INVALID, "unknown mem_kind %d", mem_kind);
    if (!ix) return fail(GBNNS_ERR_INVALID, "null index");
    if (n_q == 0) return GBNNS_OK;
    const size_t lds = rerank_topk_lds(ix->d_pad, cand_stride);
    if (lds > kMaxLds)
        return fail(GBNNS_ERR_UNSUPPORTED, "gbnns_rerank_topk: query + %u candidates' keys and distances need %zu bytes of LDS (limit %zu)",
                    cand_stride, lds, kMaxLds);
    const uint32_t nq = (uint32_t)n_q;
    const bool host = mem_kind == GBNNS_MEM_HOST;
    if (host) {
        for (uint64_t i = 0; i < n_q; ++i) {
            const uint32_t c = count ? (uint32_t)std::max(count[i], 0) : cand_stride;
            if (c > cand_stride) return fail(GBNNS_ERR_INVALID, "count[%llu] > stride", (unsigned long long)i);
            for (uint32_t j = 0; j < c; ++j)
                if (cand[i * cand_stride + j] >= ix->n)
                    return fail(GBNNS_ERR_INVALID, "candidate id %u >= n", cand[i * cand_stride + j]);
        }
    }
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc;
    if ((rc = enter_stream(ix, s))) return rc;
    Lane& L = ix->lanes[0];
    RerankTopkParams r{};
    r.dstride = ix->d_pad; r.dim = ix->d; r.qstride = ix->d; r.cand_stride = cand_stride;  // (r.db: rerank_launch, by the handle's row kind)
    r.nq = nq; r.n = (uint32_t)ix->n; r.k = (uint32_t)k;
    if ((rc = L.cnt.ensure((size_t)nq * 4))) return rc;
    int32_t* cnt_dev = L.cnt.as<int32_t>();
    const size_t bk = (size_t)nq * k * 4;
    if (host) {
        if ((rc = L.q_in.ensure((size_t)nq * ix->d * 4))) return rc;
        if ((rc = L.cand.ensure((size_t)nq * cand_stride * 4))) return rc;
        if ((rc = L.top_ids.ensure(bk))) return rc;
        if (out_dist && (rc = L.top_dist.ensure(bk))) return rc;
        if ((rc = host_copy_in(L, L.q_in.p, queries, (size_t)nq * ix->d * 4, s))) return rc;
        if ((rc = host_copy_in(L, L.cand.p, cand, (size_t)nq * cand_stride * 4, s))) return rc;
        if (count && (rc = host_copy_in(L, cnt_dev, count, (size_t)nq * 4, s))) return rc;
        r.q = L.q_in.as<float>(); r.cand = L.cand.as<uint32_t>(); r.out = L.top_ids.as<uint32_t>();
        r.out_dist = out_dist ? L.top_dist.as<float>() : nullptr;
    } else {
        r.q = queries; r.cand = cand; r.out = out_ids; r.out_dist = out_dist;
        if (count) cnt_dev = const_cast<int32_t*>(count);
    }
    if (!count) HIP_TRY(launch_fill_u32(reinterpret_cast<uint32_t*>(cnt_dev), cand_stride, nq, s));
    r.count = cnt_dev;
    HIP_TRY(rerank_launch(ix, r, s));
    if (host) {
        if ((rc = host_copy_out(L, out_ids, r.out, bk, bk, 1, s))) return rc;
        if (out_dist && (rc = host_copy_out(L, out_dist, r.out_dist, bk, bk, 1, s))) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        ix->in_flight = false;
    }
    return GBNNS_OK;
}

}  // extern "C"
