"""The census of the projection kernel instances: one static table of MODE_NET searches that, between them, launch every reachable
instance of mlp_net_kernel (16), mlp_slab_kernel (16 of 20), the per-layer kernels of mlp.hip (scalar 3, vec 3, sw 1 of 2, narrow 2 of 3,
mfma 2, normalize_kernel) and mlp_mfma_net_kernel (3), and the data those searches run on.  A plain module:
tests/test_projection_instances_cpu.py proves on the CPU, through gbnns_debug_project_plan, that every case launches the instances it
names and that the names cover the instance list exactly; tests/test_gpu_projection_instances.py runs every case on the device, q_low bit
for bit against the CPU oracle (the matrix-core option: within its promise).

A case is what a caller can set -- d, d_hidden, d_low, n_q, a plain call or three deferred calls in flight, the handle knobs "mlp_net" /
"mlp_slab" / "mlp_small", FLAG_MFMA_PROJECTION -- plus the names that must come out, in launch order.  The tables below restate the launch
rules of run_project, launch_mlp_net, slab_shape / mlp_slab_wins, launch_mlp_layer and launch_mlp_mfma_net by hand, for a device of 256
compute units: that is the point.

Shapes, the smallest at which an instance can still go wrong:
  n_q, one-launch kernel   a workgroup holds Q = 8 A queries (half-CU form: 4 A), and A is the strip that needs the fewest rounds of 256
                CUs: A = 2 from 2 048 queries (the least batch the kernel serves), 3 from 4 097, 4 from 6 145, 5 from 8 193.  The batches
                2 061 / 4 099 / 6 157 / 8 230 sit a little above those, with a last workgroup that is partial and whose length is no
                multiple of the 8 (4) query groups of a lane row; 2 048 is the whole-blocks-only batch of either form.
  n_q, matrix-core net     a workgroup holds ceil(n_q / 256) queries in RB = 1 .. 3 row blocks of 16: 2 066 gives 9 queries (RB = 1), 6 667
                gives 27 (RB = 2) and 10 765 gives 43 (RB = 3) -- the last row block holds 11 rows, enough for the copies of copy_rows --,
                the last workgroup partial every time; 8 230 (33 queries, RB = 3) is the SIFT net's batch.
  n_q, slab kernel         a wide layer (more than 64 neurons, gy = ceil(d_out / 128) columns of workgroups) takes strips of 8 A queries
                with A the cheapest of 2 .. 5 and runs on the slab kernel while ceil(n_q / 8 A) gy <= 256: gy = 4 (512 neurons) gives
                A = 2 up to 1 024 queries, 3 to 1 536, 4 to 2 048, 5 to 2 560 (1 003 / 1 301 / 1 803 / 2 303: partial last strips); gy = 2
                twice and gy = 1 four times those.  A narrow layer (<= 32 neurons: 2 wavefronts, <= 64: 4) takes A = 1 up to 2 048
                queries and A = 2 up to 4 096.  Layers of fewer than 64 inputs never take it.
  n_q, per-layer kernels   165: six tiles of 32 queries (three of the 64 of the sw and mfma kernels), the last one partial.
  widths        d and d_hidden 40 / 72 / 136 (d % 16 == 8, no multiple of a 128-neuron pass or of a chunk of 32 or 64 inputs) and
                64 / 128 / 256 / 512 (whole passes and chunks); d_hidden 264 = two passes and 8 neurons; d_hidden <= 32 for the narrow
                kernel's ReLU form; d = 45, d_hidden = 70 (d % 4 != 0, d_hidden % 4 != 0) for the scalar kernels; d = 46 and the 4 MB net
                72 -> 1 024 for the matrix-core layer kernel (the one-launch matrix-core kernel takes neither).
  d_low         16 and 32: B3 = 2 (16: half of the pass is padding); 48 and 64: B3 = 4; 72: a second last-layer pass that is mostly
                padding, 128: two full passes; 46: d_low % 4 != 0, normalizeVector leaves the last two outputs out of the norm.  Beyond
                64 the per-layer and slab kernels do not fuse normalizeVector: normalize_kernel is a launch of its own.
  128 -> 256 -> 256 -> 32   the SIFT net, once per form at A = 5 and once at RB = 3: the instances the benchmark runs on.
"""
import collections
import functools

import numpy as np

import datagen

CUS = 256            # the table is written for a device of 256 compute units
N = 1000             # base rows
EF = 40
# mlp_net_kernel<NW, A, 8, B3, GO>: A -> a batch a little above the least one of the class
NET_NQ = {2: 2061, 3: 4099, 4: 6157, 5: 8230}
NET_WHOLE_BLOCKS = 2048
# mlp_mfma_net_kernel<RB>
MFMA_NQ = {1: 2066, 2: 6667, 3: 10765}
# mlp_slab_kernel<8, A, ...> over gy columns: A -> most queries of the class (8 A floor(256 / gy)); the case batches
SLAB_WIDE_MAX = {gy: {a: 8 * a * (256 // gy) for a in (2, 3, 4, 5)} for gy in (1, 2, 4)}
SLAB_NARROW_MAX = {1: 2048, 2: 4096}
SLAB_NQ4 = {2: 1003, 3: 1301, 4: 1803, 5: 2303}     # gy = 4
SMALL_NQ = 165

Case = collections.namedtuple("Case", "d dh dl nq flight mfma knobs names")


def _id(c):
    return "%d_%d_%d_nq%d%s%s%s" % (c.d, c.dh, c.dl, c.nq, "_flight" if c.flight else "", "_mfma" if c.mfma else "",
                                     "".join("_%s%d" % (k[4:], v) for k, v in c.knobs))


Case.id = property(_id)
Case.knob_dict = property(lambda c: dict(c.knobs))


def _b(v):
    return "true" if v else "false"


def net(half, a, dl):
    """B3: two neurons per lane group cover 32 outputs a pass, four 64."""
    return "mlp_net_kernel<%d, %d, 8, %d, %d>" % (4 if half else 8, a, 2 if dl <= 32 else 4, 4 if half else 2)


def slab(nw, a, relu, norm):
    return "mlp_slab_kernel<%d, %d, %s, %s>" % (nw, a, _b(relu), _b(norm))


def layer(relu, norm=False):
    return "mlp_layer_kernel<%s, %s>" % (_b(relu), _b(norm))


def vec(relu, norm=False):
    return "mlp_layer_vec_kernel<%s, %s>" % (_b(relu), _b(norm))


def narrow(relu, norm=False):
    return "mlp_narrow_kernel<%s, %s>" % (_b(relu), _b(norm))


SW, SW_NO_RELU = "mlp_layer_sw_kernel<true>", "mlp_layer_sw_kernel<false>"
MFMA_RELU, MFMA_LAST = "mlp_layer_mfma_kernel<true>", "mlp_layer_mfma_kernel<false>"
NORMALIZE = "normalize_kernel"


def mfma_net(rb):
    return "mlp_mfma_net_kernel<%d>" % rb


def _table():
    t = []
    off, layers = (("mlp_net", 0),), (("mlp_net", 0), ("mlp_slab", 0))
    # ---- mlp_net_kernel: plain calls the whole-CU form, calls in flight the half-CU form; per (form, A) one d_low of either B3 ----
    nets = {  # (half, A) -> nets (d, dh, dl)
        (0, 2): ((40, 72, 16), (64, 128, 48)), (0, 3): ((136, 72, 32), (40, 128, 128)), (0, 4): ((64, 264, 16), (72, 136, 72)),
        (0, 5): ((128, 256, 32), (40, 72, 64)),
        (1, 2): ((40, 72, 32), (64, 128, 72)), (1, 3): ((64, 136, 16), (40, 72, 46)), (1, 4): ((136, 72, 32), (40, 128, 128)),
        (1, 5): ((128, 256, 32), (72, 128, 48)),
    }
    for (half, a), shapes in nets.items():
        for d, dh, dl in shapes:
            t.append(Case(d, dh, dl, NET_NQ[a], bool(half), False, (), (net(half, a, dl),)))
    t.append(Case(72, 136, 64, NET_WHOLE_BLOCKS, False, False, (), (net(0, 2, 64),)))
    t.append(Case(72, 136, 16, NET_WHOLE_BLOCKS, True, False, (), (net(1, 2, 16),)))
    # ---- mlp_slab_kernel ----
    # 64 -> 512 -> 512 -> 32, a net the one-launch kernel refuses (its strips of 32 queries do not fit the LDS): wide A = 2 .. 5 over four columns;
    # the last layer narrow, A = 1 up to 2 048 queries and 2 beyond
    for a, nq in SLAB_NQ4.items():
        t.append(Case(64, 512, 32, nq, False, False, (), (slab(8, a, True, False),) * 2 + (slab(2, 1 if nq <= 2048 else 2, False, True),)))
    # 72 -> 136 -> 136 -> 48: two columns, a last layer of four wavefronts
    t.append(Case(72, 136, 48, 1003, False, False, (), (slab(8, 2, True, False),) * 2 + (slab(4, 1, False, True),)))
    t.append(Case(72, 136, 48, 2061, False, False, off, (slab(8, 3, True, False),) * 2 + (slab(4, 2, False, True),)))
    # narrow hidden layers (ReLU): 32 neurons, whose 32 outputs are too few inputs for the slab kernel (the narrow per-layer kernel takes
    # layers 2 and 3), and 64 neurons
    t.append(Case(64, 32, 16, 1003, False, False, (), (slab(2, 1, True, False), narrow(True), narrow(False, True))))
    t.append(Case(64, 32, 16, 2061, False, False, off, (slab(2, 2, True, False), narrow(True), narrow(False, True))))
    t.append(Case(72, 64, 32, 1003, False, False, (), (slab(4, 1, True, False),) * 2 + (slab(2, 1, False, True),)))
    t.append(Case(72, 64, 32, 2061, False, False, off, (slab(4, 2, True, False),) * 2 + (slab(2, 2, False, True),)))
    # a wide last layer (65 .. 128 outputs, one column): no ReLU, normalizeVector in a launch of its own
    for a, nq, dl in ((2, 1003, 72), (3, 4099, 128), (4, 6157, 72), (5, 8230, 128)):
        t.append(Case(64, 128, dl, nq, False, False, off if nq >= 2048 else (), (slab(8, a, True, False),) * 2 + (slab(8, a, False, False), NORMALIZE)))
    # ---- the per-layer kernels of mlp.hip ----
    t.append(Case(40, 72, 48, SMALL_NQ, False, False, (("mlp_slab", 0),), (vec(True), vec(True), vec(False, True))))
    t.append(Case(64, 128, 72, SMALL_NQ, False, False, layers, (vec(True), vec(True), vec(False), NORMALIZE)))
    t.append(Case(45, 70, 48, SMALL_NQ, False, False, (), (layer(True), layer(True), layer(False, True))))
    t.append(Case(45, 70, 72, SMALL_NQ, False, False, (), (layer(True), layer(True), layer(False), NORMALIZE)))
    t.append(Case(40, 24, 16, SMALL_NQ, False, False, (), (narrow(True), narrow(True), narrow(False, True))))
    t.append(Case(256, 32, 32, SMALL_NQ, False, False, layers, (narrow(True), narrow(True), narrow(False, True))))
    # batches in flight of "mlp_small" .. 32 "mlp_small" queries: the small-footprint kernel for hidden layers of 64 neurons and more
    t.append(Case(64, 128, 32, SMALL_NQ, True, False, (("mlp_small", 64),), (SW, SW, narrow(False, True))))
    t.append(Case(40, 72, 48, SMALL_NQ, True, False, (("mlp_small", 64),), (SW, SW, vec(False, True))))
    # ---- the matrix-core option ----
    t.append(Case(128, 256, 32, NET_NQ[5], False, True, (), (mfma_net(3),)))
    t.append(Case(40, 72, 48, MFMA_NQ[3], False, True, (), (mfma_net(3),)))
    t.append(Case(64, 128, 32, MFMA_NQ[2], False, True, (), (mfma_net(2),)))
    t.append(Case(40, 72, 16, MFMA_NQ[2], False, True, (), (mfma_net(2),)))
    t.append(Case(64, 128, 64, MFMA_NQ[1], False, True, (), (mfma_net(1),)))
    t.append(Case(136, 72, 46, SMALL_NQ, False, True, (), (mfma_net(1),)))
    # (d % 4 != 0, and a net of more than 2 MB: the per-layer matrix-core kernel, normalizeVector always a launch of its own)
    t.append(Case(46, 72, 32, SMALL_NQ, False, True, (), (MFMA_RELU, MFMA_RELU, MFMA_LAST, NORMALIZE)))
    t.append(Case(72, 1024, 64, SMALL_NQ, False, True, (), (MFMA_RELU, MFMA_RELU, MFMA_LAST, NORMALIZE)))
    return tuple(t)


CASES = _table()

# Instances no handle call reaches: the last layer always normalises and has no ReLU, the hidden layers always have one.
UNREACHABLE = {}
for _nw in (2, 4):
    for _a in (1, 2):
        UNREACHABLE[slab(_nw, _a, False, False)] = ("a layer of up to 64 neurons is one column of workgroups, so the only layer without ReLU, the last one, "
                                                   "always normalises inside the launch (<false, true>)")
UNREACHABLE[SW_NO_RELU] = "the small-footprint kernel takes layers that do not normalise, and the only layer without ReLU is the one that does"
UNREACHABLE[narrow(False, False)] = "a layer without ReLU is the last one, which normalises (<false, true>)"


def instance_names():
    """The 53 instances of the three files, by family: the template instantiations of mlp_net.hip (net_launch_a, slab_launch), mlp.hip
    (launch_mlp_layer, launch_mlp_layer_mfma, launch_normalize) and mlp_mfma_net.hip (launch_mlp_mfma_net)."""
    tf = ((True, False), (False, True), (False, False))
    return {
        "net": {"mlp_net_kernel<%d, %d, 8, %d, %d>" % (nw, a, b3, go) for nw, go in ((8, 2), (4, 4)) for a in (2, 3, 4, 5) for b3 in (2, 4)},
        "slab": {slab(8, a, r, False) for a in (2, 3, 4, 5) for r in (True, False)} |
                {slab(nw, a, r, n) for nw in (2, 4) for a in (1, 2) for r, n in tf},
        "layer": {layer(r, n) for r, n in tf},
        "vec": {vec(r, n) for r, n in tf},
        "sw": {SW, SW_NO_RELU},
        "narrow": {narrow(r, n) for r, n in tf},
        "mfma_layer": {MFMA_RELU, MFMA_LAST},
        "mfma_net": {mfma_net(rb) for rb in (1, 2, 3)},
        "normalize": {NORMALIZE},
    }


def batches(case):
    """Calls of a case: three deferred ones in flight, or one."""
    return 3 if case.flight else 1


def mfma_rows(nq):
    """Queries per workgroup of mlp_mfma_net_kernel on 256 CUs (every net of the table holds three row blocks)."""
    return max(1, min(-(-nq // CUS), 48))


def copy_rows(nq):
    """The matrix-core cases' wrong-row-block check: (destinations, sources).  Rows 3 .. 10 of every 16-row block of workgroup 1's share,
    and of the last (partial) workgroup's, hold copies of rows 3 .. 10 of workgroup 0, as far as a share has such rows: a copy's q_low must
    equal its source's bit for bit, because an output's chain of multiply-adds does not depend on where its row sits."""
    rows = mfma_rows(nq)
    last = (nq - 1) // rows * rows
    dst, src = [], []
    for w in {rows, last} - {0}:
        for o in range(min(rows, nq - w)):
            if 3 <= o % 16 <= 10 and o % 16 < rows:
                dst.append(w + o)
                src.append(o % 16)
    return np.array(dst, np.int64), np.array(src, np.int64)


@functools.lru_cache(maxsize=4)
def data(d, dh, dl, nq_total, copies=False):
    """(base, queries, net, graph offsets, graph neighbours, entry ids) -- datagen.full_mantissa rows and datagen.net_layers_full layers:
    every product and partial sum rounds.  copies: copy_rows' queries are in place."""
    rng = np.random.Generator(np.random.PCG64(9100 + 7 * d + 3 * dh + dl))
    base = datagen.full_mantissa(rng, N, d)
    queries = datagen.full_mantissa(rng, nq_total, d)
    layers = datagen.net_layers_full(rng, d, dh, dl)
    off, nbr = datagen.random_graph(rng, N, 4, 28)
    ent = rng.integers(0, N, size=nq_total).astype(np.uint32)
    if copies:
        dst, src = copy_rows(nq_total)
        queries[dst] = queries[src]
    for a in (base, queries, ent) + tuple(layers):
        a.setflags(write=False)
    return base, queries, layers, off, nbr, ent
