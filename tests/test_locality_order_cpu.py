"""The locality order of deep batches, as far as a machine without a device can check it: the reference key and the validity check
themselves (tests/locality_order_util.py), the condition under which an ordered GPU run proves anything -- the sort must really move the
batch --, and the round trips of the handle knobs "order_min" / "order_bits" through the process-wide defaults.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import locality_order_util as lo


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def test_key_on_the_edges_of_the_float_range():
    """+-0, NaN and -inf give 0; +inf, the positive subnormals and the largest finite value give 1; coordinate 0 is the most significant bit."""
    tiny = np.float32(1e-45)
    assert tiny > 0 and tiny == np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]
    big = np.finfo(np.float32).max
    row = np.array([[0.0, -0.0, np.nan, np.inf, -np.inf, tiny, -tiny, big, -big, 1.0, -1.0, 0.0]], np.float32)
    bits = "000101010100"
    assert int(lo.key(row, 12)[0]) == int(bits, 2)
    assert int(lo.key(row, 10)[0]) == int(bits[:10], 2)
    one = np.zeros((1, 16), np.float32)
    one[0, 0] = 1
    assert int(lo.key(one, 16)[0]) == 1 << 15 and int(lo.key(one, 10)[0]) == 1 << 9
    one[0, 0], one[0, 15] = 0, 1
    assert int(lo.key(one, 16)[0]) == 1 and int(lo.key(one, 12)[0]) == 0
    nan = np.frombuffer(np.array([0x7FC00001, 0xFFC00000, 0x7F800001], np.uint32).tobytes(), np.float32)
    assert int(lo.key(np.tile(nan, 4)[None, :], 12)[0]) == 0


def test_the_validity_check_bites():
    rng = np.random.default_rng(1)
    q = rng.standard_normal((300, 16)).astype(np.float32)
    for bits in lo.BITS:
        good = lo.stable_order(q, bits)
        assert lo.problems(good, q, bits) == []
        # the order inside a bucket is free
        k = lo.key(q, bits)[good]
        same = np.flatnonzero(k[1:] == k[:-1])
        if same.size:
            swapped = good.copy()
            swapped[[same[0], same[0] + 1]] = swapped[[same[0] + 1, same[0]]]
            assert lo.problems(swapped, q, bits) == []
        dup = good.copy()
        dup[7] = dup[8]
        assert any("permutation" in p for p in lo.problems(dup, q, bits))
        out = good.copy()
        out[0] = 300
        assert any("outside" in p for p in lo.problems(out, q, bits))
        assert lo.problems(good[:-1], q, bits)
        assert any("decrease" in p for p in lo.problems(good[::-1].copy(), q, bits))
        assert any("decrease" in p for p in lo.problems(np.arange(300, dtype=np.uint32), q, bits))
    # an inclusive scan shifts every bucket by its own size: slots past the end, others never written
    assert lo.problems(np.full(300, 0xFFFFFFFF, np.uint32), q, 12)


def test_every_fixture_run_in_order_is_moved_by_the_sort(orc):
    """An ordered run equals the unordered one trivially where the sort leaves the batch as it is.  Under a stable sort at least 90 of the
    96 work items of every batch the GPU tests run in order change their query (measured: 92 .. 96), at every key width they run it at."""
    fixtures = lo.fixtures() + [lo.net_fixture(orc)]
    assert len(fixtures) >= 40
    low = []
    for name, widths, q in fixtures:
        assert q.dtype == np.float32 and q.shape[0] == 96 and q.shape[1] >= 16, (name, q.dtype, q.shape)
        for bits in widths:
            m = lo.moved(q, bits)
            print("moved", name, bits, m)
            if m < lo.MOVED_MIN:
                low.append((name, bits, m))
    assert not low, low


def test_knob_defaults_and_clamps_without_a_device(g):
    """gbnns_debug_knob sets the process-wide defaults and gbnns_index_knob_get(NULL, ...) reads them: 32 768 and 12 out of the box,
    order_bits clamped to 10 .. 16, a negative order_min counts as never.  In a child process: a default set here would be every later
    handle's."""
    script = ("import sys\n"
              "sys.path.insert(0, sys.argv[1])\n"
              "import gbnns_dim_red_amd as g\n"
              "lib = g.load_library()\n"
              "print(g.knob_default('order_min'), g.knob_default('order_bits'))\n"
              "for name, v in (('order_bits', 9), ('order_bits', 17), ('order_bits', 16), ('order_bits', 10), ('order_bits', -3),\n"
              "                ('order_min', -1), ('order_min', 0), ('order_min', 1), ('order_min', 1 << 30)):\n"
              "    assert lib.gbnns_debug_knob(name.encode(), v) == 0\n"
              "    print(name, v, g.knob_default(name))\n"
              "import ctypes\n"
              "v = ctypes.c_int(-7)\n"
              "print([lib.gbnns_index_knob_get(None, n, ctypes.byref(v)) for n in (b'order_last', b'cus', b'quotient', b'no_such_knob')], v.value)\n"
              "print(lib.gbnns_index_knob(None, b'order_min', 1))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("GBNNS_ORDER_MIN", "GBNNS_ORDER_BITS")}
    p = subprocess.run([sys.executable, "-c", script, root], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert lines[0] == "32768 12", lines
    assert lines[1:10] == ["order_bits 9 10", "order_bits 17 16", "order_bits 16 16", "order_bits 10 10", "order_bits -3 10",
                           "order_min -1 0", "order_min 0 0", "order_min 1 1", "order_min %d %d" % (1 << 30, 1 << 30)], lines
    assert lines[10] == "[1, 1, 1, 1] -7" and lines[11] == "1", lines


@pytest.mark.parametrize("env_min,env_bits,want", [("4096", "16", "4096 16"), ("0", "9", "0 10"), ("-5", "40", "0 16")])
def test_the_environment_variables_are_the_defaults(g, env_min, env_bits, want):
    script = ("import sys\n"
              "sys.path.insert(0, sys.argv[1])\n"
              "import gbnns_dim_red_amd as g\n"
              "g.load_library()\n"
              "print(g.knob_default('order_min'), g.knob_default('order_bits'))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GBNNS_ORDER_MIN=env_min, GBNNS_ORDER_BITS=env_bits)
    p = subprocess.run([sys.executable, "-c", script, root], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip() == want, p.stdout


def test_exports_and_refusals_without_a_device(g):
    from gbnns_dim_red_amd import binding
    lib = g.load_library()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gbnns.h")).read()
    for name in ("gbnns_index_order_last", "gbnns_debug_query_order"):
        assert name in binding.SYMBOLS and hasattr(lib, name) and ("int %s(" % name) in header, name
    assert callable(g.query_order) and callable(g.knob_default) and callable(g.Index.order_last)
    q, out = np.ones((4, 16), np.float32), np.zeros(4, np.uint32)
    call = lambda *a: lib.gbnns_debug_query_order(*a)
    assert call(None, 16, 16, 4, 12, out.ctypes.data) == 1 and call(q.ctypes.data, 16, 16, 4, 12, None) == 1
    assert call(q.ctypes.data, 16, 0, 4, 12, out.ctypes.data) == 1      # no coordinates
    assert call(q.ctypes.data, 8, 16, 4, 12, out.ctypes.data) == 1       # rows closer together than they are long
    assert call(q.ctypes.data, 16, 16, 0, 12, out.ctypes.data) == 1      # no queries
    assert call(q.ctypes.data, 16, 16, 1 << 31, 12, out.ctypes.data) == 1
    assert call(q.ctypes.data, 16, 16, 4, -1, out.ctypes.data) == 1
    assert not out.any()
    import ctypes
    n = ctypes.c_uint64(9)
    assert lib.gbnns_index_order_last(None, out.ctypes.data, 4, ctypes.byref(n)) == 1 and n.value == 9
