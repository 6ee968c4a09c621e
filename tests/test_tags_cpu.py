"""gbnns_search_tagged without a device: the exports, the plan of a tagged call, cut_graph (the NumPy definition of G'), and the fixtures
of tests/test_gpu_tags.py -- on each of them the oracle's walk on G' differs from its walk on the full graph, so a kernel that ignored
the tags cannot pass there.
"""
import numpy as np
import pytest

import tag_util as tg
import topk_util as tu


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_exports(g):
    from gbnns_dim_red_amd import binding
    for name in ("gbnns_index_set_tags", "gbnns_search_tagged", "gbnns_debug_tag_plan"):
        assert name in binding.SYMBOLS and hasattr(g.load_library(), name), name
    assert callable(g.cut_graph) and hasattr(g.Index, "set_tags") and hasattr(g.Index, "clear_tags")


@pytest.mark.parametrize("one_pass", [True, False], ids=["one_pass", "two_pass"])
def test_tag_plan_names_every_instance(g, one_pass):
    """Every (shape, beam) of the GPU tests: adjacency rows of 32 slots (the contest graphs) and of 48 (the two-pass graph)."""
    stride = 32 if one_pass else 48
    for metric, dlow in tg.TWO_PASS_SHAPES:
        for ef in tg.BEAMS:
            assert g.tag_plan(metric, dlow, tg.N, stride, ef) == tg.tag_kernel(metric, dlow, ef, one_pass), (metric, dlow, ef)


def test_tag_plan_outside_the_domain_is_the_general_kernel(g):
    for ef in (8, 64, 100, 200):
        assert g.tag_plan(0, 32, tg.N, 32, ef, aux_stride=16) == "walk_general_kernel"
        assert g.tag_plan(0, 32, tg.N, 32, ef, n_entries=2) == "walk_general_kernel"
        assert g.tag_plan(0, 32, tg.N, 32, ef, wide=True) == "walk_general_kernel"
    assert g.tag_plan(0, 32, tg.N, 32, 1100) == "walk_general_kernel"      # the LDS-list beams
    assert g.tag_plan(0, 128, tg.N, 32, 64) == "walk_general_kernel"       # a PLAIN walk over 512-byte rows
    assert g.tag_plan(1, 48, tg.N, 32, 64) == "walk_general_kernel"        # the negative dot over other widths
    assert g.tag_plan(0, 30, tg.N, 32, 64) == "walk_general_kernel"        # padded rows
    assert g.tag_plan(0, 32, 1 << 24, 32, 64) == "walk_general_kernel"     # ids beyond 24 bits
    with pytest.raises(g.GbnnsError):
        g.tag_plan(0, 32, tg.N, 33, 64)


def test_untagged_plan_is_unchanged(g):
    """The tag table is asked for tagged plans only: gbnns_debug_walk_plan still names the untagged instances."""
    import ctypes as C
    name, lds = C.create_string_buffer(128), C.c_uint64(0)
    for ef, want in ((64, "walk_hot_kernel"), (200, "walk_hot_big_kernel")):
        assert g.load_library().gbnns_debug_walk_plan(0, 32, 32, tg.N, 32, 0, ef, 1, 0, 0, 0, 0, 0, 0, name, 128, C.byref(lds)) == 0
        assert name.value.decode().startswith(want), name.value


def test_cut_graph_keeps_order_and_drops_exactly_the_disallowed(g):
    rng = tu.rng_of(9400)
    c = tg.two_pass(0, 32)
    off, nbr = c["off"], c["nbr"]
    for frac in (0.0, 0.125, 0.5, 1.0):
        allowed = rng.random(tg.N) < frac
        o2, n2 = g.cut_graph(off, nbr, allowed)
        assert o2.dtype == np.uint64 and n2.dtype == np.uint32 and len(o2) == tg.N + 1 and o2[0] == 0 and o2[-1] == len(n2)
        for i in range(tg.N):
            row = nbr[int(off[i]):int(off[i + 1])]
            assert np.array_equal(n2[int(o2[i]):int(o2[i + 1])], row[allowed[row]]), (frac, i)
    with pytest.raises(ValueError):
        g.cut_graph(off, nbr, np.ones(tg.N - 1, bool))


def test_walk_on_the_uncut_graph_is_the_walk(g, orc):
    c = tg.two_pass(0, 32)
    off, nbr = g.cut_graph(c["off"], c["nbr"], np.ones(tg.N, bool))
    assert np.array_equal(off, c["off"]) and np.array_equal(nbr, c["nbr"])
    a = orc.walk(c["q_low"], c["db_low"], off, nbr, 64, entries=c["ent"], threads=4)
    b = orc.walk(c["q_low"], c["db_low"], c["off"], c["nbr"], 64, entries=c["ent"], threads=4)
    for name in a:
        assert a[name].tobytes() == b[name].tobytes(), name
    all_q = np.full(tg.NQ, tg.ALL, np.uint32)
    e = tg.expected(orc, c, 64, 0, T=np.full(tg.N, tg.ALL, np.uint32), Q=all_q)
    assert np.array_equal(e["ids"], b["ids"]) and np.array_equal(e["hops"], b["hops"])


def test_fixtures_are_not_vacuous(orc):
    """On every fixture and beam of the bit-for-bit GPU test the expected answer or hop count on G' differs from the full graph's for at
    least a quarter of the queries with Q != all; every entry point is allowed; the three values of Q allow about 1/2, 1/8 and all rows."""
    T = tg.row_tags()
    frac = [float(((T & q) != 0).mean()) for q in tg.Q_VALUES]
    assert 0.4 < frac[0] < 0.6 and 0.08 < frac[1] < 0.17 and frac[2] == 1.0, frac
    cases = [(tg.contest(m, d, dl), m) for m, d, dl in tg.SHAPES] + [(tg.two_pass(m, dl), m) for m, dl in tg.TWO_PASS_SHAPES]
    for c, metric in cases:
        assert tg.entry_ok(c["T"], c["Q"], c["ent"]).all()
        for ef in tg.BEAMS:
            differ, of = tg.restricted_queries_that_differ(tg.expected(orc, c, ef, metric), tg.untagged(orc, c, ef, metric), c["Q"])
            assert 4 * differ >= of > 0, (metric, c["db_low"].shape, ef, differ, of)


def test_odd_first_graphs_walk_through_the_even_tail(orc):
    """The hand-built graphs: on G' every query fills its beam through the 8 even neighbours behind a row's odd ones."""
    for slots in (40, 72):
        c = tg.odd_first(slots)
        deg = np.diff(c["off"].astype(np.int64))
        assert (deg == slots).all() and (c["nbr"].reshape(tg.N, slots)[:, :slots - 8] % 2 == 1).all() and (c["nbr"].reshape(tg.N, slots)[:, slots - 8:] % 2 == 0).all()
        for ef in (8, 100, 200):
            e = tg.expected(orc, c, ef, 0)
            assert (e["count"] == ef).all() and (e["hops"] >= ef).all() and (e["ids"] % 2 == 0).all()


def test_bad_entry_rows_of_the_expected_values(orc):
    c = tg.contest(0, 128, 32)
    Q, ent = c["Q"].copy(), c["ent"].copy()
    Q[5] = 0
    ent[7] = tg.N + 3
    e = tg.expected(orc, c, 8, 0, Q=Q, ent=ent)
    for i in (5, 7):
        assert (e["ids"][i] == tg.NONE).all() and np.isinf(e["dists"][i]).all() and e["count"][i] == e["hops"][i] == e["dist_calc"][i] == 0
        assert e["want"][i] == tg.NONE


def test_one_pass_tag_instances_wait_for_the_tags_alone(tmp_path):
    """The order DESIGN.md describes, read off the shipped code object: in the hop of every tag instance over one-pass adjacency rows (rows of
    8 / 12 / 16 steps) the lane's row loads (STEPS / 2 of 16 bytes) are issued behind the tag load and ahead of the wait the tag test needs,
    and that wait leaves exactly those loads in flight -- the tag test waits for the tags alone."""
    import os
    import re
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib, objdump = os.path.join(root, "gbnns_dim_red_amd", "lib", "libgbnns_hip.so"), "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump of the ROCm toolchain not found")
    copy = shutil.copy(lib, tmp_path)
    subprocess.run([objdump, "--offloading", copy], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    kernels, name = {}, None
    for f in os.listdir(tmp_path):
        if not f.endswith("gfx950"):
            continue
        text = subprocess.run([objdump, "-d", "--no-show-raw-insn", os.path.join(tmp_path, f)], check=True, capture_output=True, text=True).stdout
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                name = m.group(1) if re.search(r"walk_reg_(big_)?tag_kernel", m.group(1)) else None
                if name:
                    kernels[name] = []
            elif name and line.startswith("\t"):
                kernels[name].append(line.strip().split("//")[0].strip())
    assert len(kernels) == 24, sorted(kernels)
    checked = 0
    for name, ins in kernels.items():
        m = re.search(r"walk_reg_tag_kernelILi\dELi(8|12|16)ELi1ELb1E|walk_reg_big_tag_kernelILi\dELi(8|12|16)ELb1ELb0E", name)
        if not m:
            continue
        steps = int(m.group(1) or m.group(2))
        # the tag table's address: WalkParams::tags, byte 408 of the kernel arguments
        base = [re.match(r"s_load_dwordx[24] s\[(\d+):\d+\], s\[0:1\], 0x198", i) for i in ins]
        base = [b.group(1) for b in base if b]
        assert len(base) == 1, (name, base)
        loads = [i for i, x in enumerate(ins) if re.match(r"global_load_dword v\d+, v\d+, s\[%s:" % base[0], x)]
        assert len(loads) == 2, (name, loads)   # the entry row's tag, the hop's
        rows, wait = 0, None
        for x in ins[loads[1] + 1:]:
            rows += x.startswith("global_load_dwordx4")
            w = re.search(r"vmcnt\((\d+)\)", x)
            if w:
                wait = int(w.group(1))
                break
        assert rows == steps // 2 and wait == steps // 2, (name, rows, wait)
        checked += 1
    assert checked == 8
