"""CPU-side checks of the C-ABI library: it builds, loads, exports every declared symbol, refuses
to run without a GPU (no CPU fallback), and its host-side graph builder matches the reference."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import datagen
import golden_util as gu
import gbnns_dim_red_amd as g
from gbnns_dim_red_amd import binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    g.build_library()
    return g.load_library()


def test_exports_every_declared_symbol(lib):
    header = open(os.path.join(ROOT, "include", "gbnns.h")).read()
    declared = set(re.findall(r"^(?:int|void|void\*|const char\*|uint64_t|uint32_t|gbnns_index\*)\s+(gbnns_[a-z_0-9]+)\s*\(",
                              header, re.M))
    assert declared == set(binding.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), name
    assert g.version() == 100


def test_struct_sizes_match_header(lib):
    # 8-byte aligned C layouts as declared in include/gbnns.h
    assert ctypes.sizeof(binding._IndexDesc) == 96
    assert ctypes.sizeof(binding._SearchArgs) == 136  # + n_entries, defer_depth
    assert ctypes.sizeof(binding.Profile) == 304  # + walk_kernel[96], project_kernel[32]; + retry_kernel[96], retry_queries, retry_general_queries


def test_shard_bounds_arithmetic(lib):
    """gbnns_shard_bounds (the block arithmetic of gbnns_multi_* and of the C++ drop-in) = sharding.shard_bounds
    (what bench.py and the gloo tests use): contiguous, covering, sizes differ by at most one."""
    from gbnns_dim_red_amd import sharding
    lib.gbnns_shard_bounds.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32,
                                       ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    lib.gbnns_shard_bounds.restype = None
    lo, hi = ctypes.c_uint64(), ctypes.c_uint64()
    for n_q in (0, 1, 7, 8, 9, 1000, 10_000, 1_000_000, 999_999, (1 << 33) + 5):
        for parts in (1, 2, 3, 4, 7, 8, 64):
            prev = 0
            sizes = []
            for part in range(parts):
                lib.gbnns_shard_bounds(n_q, parts, part, ctypes.byref(lo), ctypes.byref(hi))
                assert (lo.value, hi.value) == sharding.shard_bounds(n_q, parts, part)
                assert lo.value == prev and hi.value >= lo.value
                prev = hi.value
                sizes.append(hi.value - lo.value)
            assert prev == n_q and max(sizes) - min(sizes) <= 1
            assert max(sizes) == sharding.shard_pad(n_q, parts)
    lib.gbnns_shard_bounds(10, 4, 9, ctypes.byref(lo), ctypes.byref(hi))  # part out of range: empty block
    assert (lo.value, hi.value) == (0, 0)


def test_multi_argument_validation(lib):
    h = ctypes.c_void_p()
    assert lib.gbnns_multi_create(None, None, 0, ctypes.byref(h)) == 1
    d = binding._IndexDesc(struct_size=ctypes.sizeof(binding._IndexDesc), mem_kind=binding.MEM_DEVICE)
    assert lib.gbnns_multi_create(ctypes.byref(d), None, 0, ctypes.byref(h)) == 1   # device tensors cannot be replicated
    lib.gbnns_multi_last_error.restype = ctypes.c_char_p
    assert b"HOST" in lib.gbnns_multi_last_error()
    assert lib.gbnns_multi_size(None) == 0
    assert lib.gbnns_multi_search_ex(None, None) == 1
    if _no_gpu():
        d.mem_kind = binding.MEM_HOST
        assert lib.gbnns_multi_create(ctypes.byref(d), None, 0, ctypes.byref(h)) == 2  # no device, no CPU path


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.skipif(not _no_gpu(), reason="only meaningful on a box without a GPU")
def test_no_cpu_fallback(lib):
    db = np.zeros((4, 8), np.float32)
    off = np.arange(5, dtype=np.uint64)
    nbr = np.array([1, 2, 3, 0], np.uint32)
    with pytest.raises(g.GbnnsError) as e:
        g.Index(db, off, nbr)
    assert e.value.code == 2  # GBNNS_ERR_NO_DEVICE


def test_argument_validation(lib):
    h = ctypes.c_void_p()
    assert lib.gbnns_index_create(None, ctypes.byref(h)) == 1
    d = binding._IndexDesc(struct_size=3)
    assert lib.gbnns_index_create(ctypes.byref(d), ctypes.byref(h)) == 1
    assert b"struct_size" in lib.gbnns_last_error()


def test_debug_knob_names(lib):
    """gbnns_debug_knob needs no GPU: every handle knob is accepted ("coop" 2 too: clamped, the two-wavefront walk has one form),
    the removed "coop_pack" and "vs_fill2" are refused like any unknown name (GBNNS_ERR_INVALID).  In a child process: a handle
    knob set here would be the default of every handle this process creates afterwards."""
    import subprocess
    handle_knobs = {"quotient": 1, "vs_disp": 15, "max_waves": 0, "spec_min_nq": 32768, "spec_any_form": 0, "mlp_small": 4096,
                    "mlp_net": 1, "mlp_slab": 1, "late_rows": -1, "spec_tail": 50, "coop": 2}
    refused = ("coop_pack", "vs_fill2", "no_such_knob")
    script = ("import ctypes, sys\n"
              "lib = ctypes.CDLL(sys.argv[1])\n"
              "lib.gbnns_debug_knob.argtypes = [ctypes.c_char_p, ctypes.c_int]\n"
              "for a in sys.argv[2:]:\n"
              "    n, v = a.split('=')\n"
              "    print(n, lib.gbnns_debug_knob(n.encode(), int(v)))\n")
    args = ["%s=%d" % kv for kv in handle_knobs.items()] + ["%s=1" % n for n in refused]
    p = subprocess.run([sys.executable, "-c", script, binding._LIB_PATH] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    codes = dict(ln.split() for ln in p.stdout.splitlines())
    assert codes == {**{n: "0" for n in handle_knobs}, **{n: "1" for n in refused}}, codes


def test_exact_knn_argument_validation(lib):
    base = np.zeros((8, 200), np.float32)
    ids = np.zeros((8, 3), np.uint32)

    def call(n, nq, d, k, metric, self_offset=-1, mem=0, b=base, out=ids):
        return lib.gbnns_exact_knn(0, b.ctypes.data if b is not None else None, n, base.ctypes.data, nq, d, k,
                                   metric, self_offset, out.ctypes.data if out is not None else None, None, mem, None)
    assert call(8, 8, 16, 3, 0, b=None) == 1          # null pointer
    assert call(0, 8, 16, 3, 0) == 1                  # empty base
    assert call(8, 8, 16, 0, 0) == 1                  # k < 1
    assert call(8, 8, 16, 3, 7) == 1                  # unknown metric
    assert call(8, 8, 16, 3, 0, mem=5) == 1           # unknown memory kind
    assert call(8, 8, 16, 3, 0, self_offset=-2) == 1
    assert call(8, 8, 9000, 3, 0) == 5                # d > 8192: GBNNS_ERR_UNSUPPORTED
    assert b"d <= 8192" in lib.gbnns_last_error()
    assert call(8, 8, 12, 3, 1) == 5                  # dot form needs d % 8 == 0
    if _no_gpu():
        assert call(8, 8, 16, 3, 0) == 2              # valid request, no device: no CPU path
    assert lib.gbnns_index_set_aux_graph(None, None, None) == 1


def test_graph_builder_matches_reference_golden(lib):
    gd = gu.load("tail_toy")
    # db_low bytes are pinned by sha in the golden; regenerate through the fixture's q_low path is
    # GPU-only, so here the builder is checked on the original-space vectors against the oracle
    # restatement (itself pinned to the reference) ...
    import oracle
    orc = oracle.Oracle()
    c = gd.case
    db_low = orc.project(c.net, c.base)
    assert datagen.sha(db_low) == gd.meta["db_low_sha"]
    koff, knbr = datagen.dense_to_csr(gd["knn"])
    for threads in (1, 3):
        off, nbr = g.build_graph_gd(koff, knbr, db_low, gd.meta["gd_M"], threads=threads)
        # ... and directly against the graph the compiled reference produced
        assert np.array_equal(off, gd["graph_off"])
        assert np.array_equal(nbr, gd["graph_nbr"])


@pytest.mark.parametrize("M,rev", [(8, True), (14, False), (5, True), (2, True)])
def test_graph_builder_vs_oracle(lib, orc, M, rev):
    c = datagen.Case("b", 78, 1200, 8, 24, 12, 16)
    knn = datagen.knn_bruteforce(c.base, 18)
    koff, knbr = datagen.dense_to_csr(knn)
    a = g.build_graph_gd(koff, knbr, c.base, M, reverse=rev, threads=4)
    b = orc.hnswlike_gd(koff, knbr, c.base, M, reverse=rev, threads=2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_bench_launches_its_own_workers():
    """`python bench.py --gpus N` without WORLD_SIZE (how the driver calls it) must start N workers itself: the launch
    command, and -- with the --launch-probe hook, which needs no GPU -- the whole path: two fresh processes, a gloo
    rendezvous on 127.0.0.1, one JSON line from rank 0, exit status of the workers."""
    import json
    import subprocess
    import bench
    assert bench.launcher_command(1, ["--gpus", "1"], {}) is None
    assert bench.launcher_command(8, ["--gpus", "8"], {"WORLD_SIZE": "8"}) is None  # already a worker
    cmd = bench.launcher_command(8, ["--gpus", "8", "--steps", "5"], {})
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "8"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[-1].endswith("bench.py")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-probe"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0]) == {"launch_probe": True, "ranks_seen": 2, "world_size": 2}
    # a failing worker's status is the launcher's status
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--launch-probe"],
                       env=dict(env, GBNNS_PROBE_FAIL_RANK="1"), capture_output=True, text=True, timeout=300)
    assert p.returncode != 0


def test_rccl_load_failure_is_an_error_not_a_crash(lib):
    """gbnns_multi_search_device loads librccl on first use with more than one replica.  When the library cannot be
    loaded the call must fail with GBNNS_ERR_UNSUPPORTED and a message (the first formulation called dlerror() twice
    and handed NULL to std::string).  GBNNS_RCCL_LIB points the loader at a file that does not exist."""
    lib.gbnns_multi_last_error.restype = ctypes.c_char_p
    old = os.environ.get("GBNNS_RCCL_LIB")
    os.environ["GBNNS_RCCL_LIB"] = "/nonexistent/librccl_missing.so"
    try:
        assert lib.gbnns_internal_rccl_probe() == 5  # GBNNS_ERR_UNSUPPORTED
        msg = lib.gbnns_multi_last_error().decode()
        assert "RCCL unavailable" in msg and "librccl_missing" in msg
    finally:
        if old is None:
            os.environ.pop("GBNNS_RCCL_LIB")
        else:
            os.environ["GBNNS_RCCL_LIB"] = old


def _walk_plan(lib, metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries, force_wide, coop, late_rows, spec_rows, pas, rr_reserve):
    name = ctypes.create_string_buffer(128)
    lds = ctypes.c_uint64()
    rc = lib.gbnns_debug_walk_plan(metric, dim, dstride, n, ell_stride, aux_stride, ef, n_entries, force_wide, coop, late_rows, spec_rows, pas,
                                   rr_reserve, name, 128, ctypes.byref(lds))
    return rc, name.value.decode(), lds.value


def test_walk_plan_over_every_shape(lib):
    """The full cross product of the plan's inputs, indexes of 2^24 rows and more and tables of 4 GiB and more included (no small GPU
    case reaches those): every shape gets a plan; its LDS without the visited set leaves room for the smallest visited set (128 4-byte
    slots) inside the 160 KB of a CU -- beams of up to 4 096, one entry point: what search_core does not send to the general kernel
    outright --; the retry plan of a shape is a retry instance and keeps the first pass's visited-set packing (compact 24-bit ids or
    4-byte slots: the retry pass is sized for the form the first pass's hand-overs were counted in); inputs no index can have are refused."""
    import itertools

    def packed(name):   # which visited-set packing the instance's name says: walk_fast_kernel<M, S, RETRY, PACKED>, <M, S, OFF32, ...>
        args = name[name.index("<") + 1:-1].split(", ") if "<" in name else []
        if name.startswith("walk_fast_kernel<"):
            return args[3] == "true"
        if name.startswith(("walk_reg_kernel<", "walk_reg_big_kernel<")):
            return args[2] == "true"
        assert name.startswith(("walk_hot", "walk_coop_kernel<", "walk_reg_wide_kernel<")), name  # compact indexes only
        return True

    def is_retry(name):
        args = name[name.index("<") + 1:-1].split(", ")
        return args[2 if name.startswith("walk_fast_kernel<") else 3] == "true"

    count = 0
    for metric, dim, n, ell, aux, ef in itertools.product((0, 1), (8, 16, 30, 32, 48, 64, 96, 128, 132, 144, 300, 960),
                                                          (3000, 0xFEFFFF, 0xFFFFFF, 1 << 24, 1 << 26, 0xFFFFFFFF), (16, 32, 64, 80), (0, 16),
                                                          (1, 8, 64, 65, 128, 129, 200, 201, 512, 1024, 1100, 4096)):
        dstride = (dim + 3) // 4 * 4
        for n_ent, wide, coop, late, spec in itertools.product((1, 3), (0, 1), (0, 1), (0, 1), (0, 1)):
            shape = (metric, dim, dstride, n, ell, aux, ef, n_ent, wide, coop, late, spec)
            rc0, first, lds0 = _walk_plan(lib, *shape, 0, 0)
            rc1, bitmap, lds1 = _walk_plan(lib, *shape, 1, 4 * 960)
            rc2, retry, lds2 = _walk_plan(lib, *shape, 2, 0)
            count += 3
            assert (rc0, rc1, rc2) == (0, 0, 0) and first and bitmap and retry, shape
            if n_ent > 1:
                assert first == "walk_general_kernel", shape
                continue
            assert max(lds0, lds1, lds2) + 128 * 4 <= 160 * 1024, (shape, lds0, lds1, lds2)
            assert first.startswith("walk_") and bitmap.startswith("walk_bitmap_") and is_retry(retry), (shape, first, bitmap, retry)
            assert packed(first) == packed(retry), (shape, first, retry)
    assert count > 1_000_000
    # refused: unknown metric, no dimension, a row stride that is not the padded dimension, no rows, more rows than ids, adjacency
    # strides that are no multiple of 16, no beam, an unknown pass
    ok = (0, 32, 32, 3000, 32, 0, 64, 1, 0, 0, 0, 0, 0, 0)
    assert _walk_plan(lib, *ok)[0] == 0
    for i, v in ((0, 2), (1, 0), (2, 36), (3, 0), (3, 1 << 32), (4, 0), (4, 40), (5, 8), (6, 0), (12, 3)):
        bad = list(ok)
        bad[i] = v
        assert _walk_plan(lib, *bad)[0] == 1, bad


def test_walk_plan_equals_the_launchers_it_replaced(lib):
    """tests/golden/walk_launches_before_plan.tsv.gz: what the launchers launched when the choice of instance still lived in them -- that
    commit's object files, driven without a device over the cross product of both metrics, walked rows of 8 .. 960 floats, indexes of
    3 000, 2^24 - 1 (tables of 4 GiB and more from 300 floats a row on) and 2^24 rows, adjacency rows of one pass, two passes and more
    than 64 slots, with and without the auxiliary graph, beams of 1 .. 1 100, forced-wide indexes, the two-wavefront walk, late and
    speculative rows, for the first, the bitmap and the retry pass (the file's header says how).  For every row the plan names the
    kernel that was launched, with the same LDS besides the visited set; no row is left out, and all 210 walk instances of the first,
    bitmap and retry passes occur."""
    import gzip
    with gzip.open(os.path.join(ROOT, "tests", "golden", "walk_launches_before_plan.tsv.gz"), "rt") as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f if not ln.startswith("#")]
    assert len(rows) == 104544 and all(len(r) == 16 for r in rows)
    assert len({r[15] for r in rows}) == 210 and {r[12] for r in rows} == {"0", "1", "2"}
    for r in rows:
        rc, name, lds = _walk_plan(lib, *(int(v) for v in r[:14]))
        assert (rc, name, lds) == (0, r[15], int(r[14])), (r, rc, name, lds)


def _golden_walk_names():
    import gzip
    with gzip.open(os.path.join(ROOT, "tests", "golden", "walk_launches_before_plan.tsv.gz"), "rt") as f:
        return {ln.rstrip("\n").split("\t")[15] for ln in f if not ln.startswith("#")}


def test_walk_instance_table_covers_every_instance(lib):
    """tests/walk_instances.py, the case table of the device census (tests/test_gpu_walk_instances.py): for every case the plan, asked
    with the decisions a search of that case resolves, names the case's `first` (first or bitmap pass) and -- hash_capacity != 0 --
    `retry` instance; the union of those names IS the set of the 210 instances of the golden file, none missing and none unknown, so
    every instance is the target of at least one case; the table stays a census (at most 260 cases) inside its own domain: the
    documented dimensions and beams, a retry case at the top of its beam class with a 128-entry visited set, speculative rows only
    with both knobs, and no two cases alike."""
    import walk_instances as wi
    golden = _golden_walk_names()
    assert len(golden) == 210
    assert len(wi.CASES) <= 260 and len(set(c[:11] for c in wi.CASES)) == len(wi.CASES)
    recorded = set()
    for c in wi.CASES:
        assert c.metric in (0, 1) and c.dim in wi.DIMS and c.deg in wi.ELL_STRIDE and c.ef in wi.BEAMS, c
        assert {c.aux, c.wide, c.bitmap, c.coop, c.late_rows, c.spec} <= {0, 1} and c.hash_capacity in (0, 128), c
        assert not (c.bitmap and (c.wide or c.coop)) and not (c.coop and c.wide), c   # (a search would not take the case as written)
        assert c.knobs["spec_tail"] == 0 and (c.knobs["spec_min_nq"], c.knobs["spec_any_form"]) in ((0, 0), (1, 1)), c
        rc, first, _ = _walk_plan(lib, *c.plan_args(c.first_pass))
        assert (rc, first) == (0, c.first), (c, rc, first)
        recorded.add(first)
        if c.hash_capacity:
            assert c.ef in (64, 128, 200, 1024, 1100), c
            assert c.ef != 1024 or ", 32, " in c.first, c   # (1 024 only where the instance serves no beam up to 200)
            rc, retry, _ = _walk_plan(lib, *c.plan_args(2))
            assert (rc, retry) == (0, c.retry), (c, rc, retry)
            recorded.add(retry)
        else:
            assert c.retry is None, c
    assert recorded == golden, (sorted(golden - recorded), sorted(recorded - golden))
    assert {c.first for c in wi.CASES} | {c.retry for c in wi.CASES if c.retry} == golden
    # short lists on every first-pass family that serves ef <= 64, as ordinary cases; one padded dimension, one beam per family
    for ef in (1, 8):
        fams = {c.first.split("<")[0] for c in wi.CASES if c.ef == ef and not c.hash_capacity}
        assert fams >= {"walk_hot_kernel", "walk_hot_spec_kernel", "walk_hotw_kernel", "walk_hot_dot_kernel", "walk_reg_wide_kernel", "walk_reg_kernel",
                        "walk_fast_kernel", "walk_bitmap_reg_kernel", "walk_bitmap_kernel"}, (ef, fams)
    padded = [c for c in wi.CASES if c.dim % 4]
    assert {c.dim for c in padded} == {30} and len({(c.metric, c.first) for c in padded}) == len(padded) == 8


def test_walk_instance_retry_cases_outgrow_their_visited_set(orc):
    """The precondition of the census's retry assertions, on the CPU: on the data of every retry case the oracle's walk computes more
    distances than the case's visited set holds (hash_capacity) for at least three quarters of the queries -- so the first pass hands at
    least that share over whatever the kernel, and "the retry pass finished half the batch" is a condition the retry instance has to
    meet, not an observation."""
    import walk_instances as wi
    retry_cases = [c for c in wi.CASES if c.hash_capacity]
    assert len({c.retry for c in retry_cases}) == 77
    for c in retry_cases:
        assert c.ef >= 64, c
        w, _ = wi.oracle_walk(orc, c)
        over = int((w["dist_calc"] > c.hash_capacity).sum())
        assert 4 * over >= 3 * wi.NQ, (c, over, int(w["dist_calc"].min()))
