"""gbnns_exact_knn_bytes without a device: the exports, the argument validation (status codes and messages, before any HIP call),
gbnns_debug_knn_bytes_plan's invariants, the binding's dispatch on the dtypes -- and the exactness claim the call rests on, by example:
on uint8 rows of d <= 256 dimensions the reference's ordered float32 sums ARE the integer distances, so the oracle over the widened
arrays, plain int64 numpy with np.lexsort((id, dist)) and an int32 matrix product agree bit for bit."""
import ctypes as C

import numpy as np
import pytest

import knn_bytes_util as ku

OK, INVALID, NO_DEVICE, UNSUPPORTED = 0, 1, 2, 5


@pytest.fixture(scope="module")
def g():
    import gbnns_dim_red_amd as g
    g.load_library()
    return g


def _no_gpu(g):
    return g.device_count() == 0   # (asked of the library itself: the same HIP runtime the call under test would use)


def test_exports(g):
    from gbnns_dim_red_amd import binding
    lib = g.load_library()
    for name in ("gbnns_exact_knn_bytes", "gbnns_debug_knn_bytes_plan"):
        assert name in binding.SYMBOLS and hasattr(lib, name), name
    assert callable(g.knn_bytes_plan)


def _call(g, base, queries, k, metric=ku.L2, self_offset=-1, n=None, n_q=None, d=None, ids=True, mem_kind=0, device=0):
    """The raw C call on host arrays; (status, message)."""
    lib = g.load_library()
    out = np.zeros((max(1, queries.shape[0] if queries is not None else 1), max(1, min(k, 8))), np.uint32)
    rc = lib.gbnns_exact_knn_bytes(device, base.ctypes.data if base is not None else None, base.shape[0] if n is None else n,
                                   queries.ctypes.data if queries is not None else None, queries.shape[0] if n_q is None else n_q,
                                   base.shape[1] if d is None else d, k, metric, self_offset, out.ctypes.data if ids else None, None,
                                   mem_kind, None)
    return rc, lib.gbnns_last_error().decode()


def test_argument_validation(g):
    """Every refusal comes before the first HIP call: the same status on a machine with and without a device."""
    b = np.zeros((8, 16), np.uint8)
    q = np.zeros((2, 16), np.uint8)
    assert _call(g, None, q, 1, n=8, d=16) == (INVALID, "null argument")
    assert _call(g, b, None, 1, n_q=2) == (INVALID, "null argument")
    assert _call(g, b, q, 1, ids=False) == (INVALID, "null argument")
    for n in (0, (1 << 32) - 1):
        rc, msg = _call(g, b, q, 1, n=n)
        assert rc == INVALID and "n must be in" in msg
    rc, msg = _call(g, b, q, 1, n_q=1 << 31)
    assert rc == INVALID and "n_q too large" in msg
    for k in (0, -1, (1 << 20) + 1):
        rc, msg = _call(g, b, q, k)
        assert rc == INVALID and "k must be in" in msg, k
    rc, msg = _call(g, b, q, 1, d=0)
    assert rc == INVALID and "d must be" in msg
    rc, msg = _call(g, b, q, 1, metric=2)
    assert rc == INVALID and "unknown metric" in msg
    rc, msg = _call(g, b, q, 1, mem_kind=7)
    assert rc == INVALID and "unknown mem_kind" in msg
    rc, msg = _call(g, b, q, 1, self_offset=-2)
    assert rc == INVALID and "self_offset" in msg
    # valid requests outside what the byte call serves: the message says why and which call does
    rc, msg = _call(g, b, q, 1, d=257)
    assert rc == UNSUPPORTED and "d <= 256" in msg and "2^24" in msg and "gbnns_exact_knn" in msg.replace("gbnns_exact_knn_bytes", "")
    rc, msg = _call(g, b, q, 4097)
    assert rc == UNSUPPORTED and "k <= 4096" in msg
    rc, msg = _call(g, np.zeros((8, 12), np.uint8), np.zeros((2, 12), np.uint8), 1, metric=ku.NEG_DOT)
    assert rc == UNSUPPORTED and "d % 8 == 0" in msg
    # ... and UNSUPPORTED wins over a bad self_offset exactly where the float call lets it
    lib = g.load_library()
    ids = np.zeros((2, 1), np.uint32)
    f = np.zeros((8, 8200), np.float32)
    assert lib.gbnns_exact_knn(0, f.ctypes.data, 8, f.ctypes.data, 2, 8200, 1, 0, -2, ids.ctypes.data, None, 0, None) == UNSUPPORTED
    assert _call(g, b, q, 1, d=257, self_offset=-2)[0] == UNSUPPORTED
    if _no_gpu(g):   # a valid request: no device, and no CPU path to fall back to
        rc, msg = _call(g, b, q, 1)
        assert rc == NO_DEVICE and "no CPU path" in msg
        with pytest.raises(g.GbnnsError) as e:
            g.exact_knn(b, q, 1)
        assert e.value.code == NO_DEVICE


@pytest.mark.parametrize("d", (1, 4, 30, 32, 33, 64, 100, 128, 192, 255, 256))
@pytest.mark.parametrize("k", (1, 10, 63, 64, 200, 4096))
def test_plan_invariants(g, d, k):
    for n in (5, 1037, 6000, 10**6):
        p = g.knn_bytes_plan(n, 300, d, k)
        assert p["dp"] % ku.K_STEP == 0 and d <= p["dp"] < d + ku.K_STEP
        assert p["cap"] >= 4 * k and p["first_rows"] <= p["cap"] and p["first_rows"] <= n
        assert p["first_rows"] == n or (p["first_rows"] % ku.ROW_BLOCK == 0 and p["first_rows"] >= k)
        assert p["max_chunk"] % ku.ROW_BLOCK == 0 and p["max_chunk"] == 4 * (1 << 15)
        assert p["pool"] == (k >= 64)
        chunks = ku.chunk_plan(p, n)
        assert sum(r for _, r in chunks) == n and chunks[0] == (0, p["first_rows"])
        for r0, rows in chunks[1:]:   # every chunk starts on a row block, is no longer than everything before it, nor than max_chunk
            assert r0 % ku.ROW_BLOCK == 0 and rows <= r0 and rows <= p["max_chunk"]


def test_plan_follows_the_knobs_and_refuses_other_shapes(g):
    with ku.knobs(g, knn_chunk=512, knn_pool_min_k=10):
        p = g.knn_bytes_plan(20000, 40, 32, 30)
        assert p["max_chunk"] == 2048 and p["pool"] is True
        assert g.knn_bytes_plan(20000, 40, 32, 9)["pool"] is False and g.knn_bytes_plan(20000, 40, 32, 10)["pool"] is True
    p = g.knn_bytes_plan(20000, 40, 32, 30)
    assert p["max_chunk"] == 4 << 15 and p["pool"] is False
    for bad in (dict(n=0), dict(d=0), dict(d=257), dict(k=0), dict(k=4097)):
        a = dict(n=100, n_q=10, d=32, k=5)
        a.update(bad)
        with pytest.raises(g.GbnnsError) as e:
            g.knn_bytes_plan(**a)
        assert e.value.code == INVALID, bad
    lib = g.load_library()
    assert lib.gbnns_debug_knn_bytes_plan(100, 10, 32, 5, None, None, None, None, None) == INVALID


class _Spy:
    """Stands in for the loaded library: records which of the two symbols a call reaches."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*a):
            self.calls.append(name)
            return 0
        return f


def test_binding_dispatch(g, monkeypatch):
    from gbnns_dim_red_amd import binding
    spy = _Spy()
    monkeypatch.setattr(binding, "load_library", lambda: spy)
    bu, qu = np.zeros((8, 16), np.uint8), np.zeros((2, 16), np.uint8)
    bf, qf = bu.astype(np.float32), qu.astype(np.float32)
    binding.exact_knn(bf, qf, 3)
    binding.exact_knn(bf.astype(np.float64), qf, 3)      # (float inputs of another width are converted, as before)
    assert spy.calls == ["gbnns_exact_knn", "gbnns_exact_knn"]
    ids, dist = binding.exact_knn(bu, qu, 3, want_dist=True)
    assert spy.calls[-1] == "gbnns_exact_knn_bytes" and ids.shape == (2, 3) and ids.dtype == np.uint32 and dist.dtype == np.float32
    for pair in ((bu, qf), (bf, qu)):
        with pytest.raises(TypeError) as e:
            binding.exact_knn(*pair, 3)
        assert "gbnns_exact_knn_bytes" in str(e.value) and "astype(float32)" in str(e.value)
    assert len(spy.calls) == 3
    import torch
    with pytest.raises(TypeError):   # a torch pair of mixed dtypes is refused before anything looks at where it lives
        binding.exact_knn(torch.zeros((8, 16), dtype=torch.uint8), torch.zeros((2, 16), dtype=torch.float32), 3)


@pytest.mark.parametrize("d", (28, 128, 256))
def test_float32_sums_of_byte_rows_are_the_integers(d):
    """The exactness claim by example, at its edge: an all-0 row against an all-255 row.  The ordered float32 four-sum (L2) and eight-sum
    (negative dot; d % 8 == 0) emulations equal the int64 sums, the largest of which, 256 * 65 025 = 16 646 400, is below 2^24."""
    lo, hi = np.zeros(d, np.uint8), np.full(d, 255, np.uint8)
    rng = np.random.default_rng(d)
    pairs = [(lo, hi), (hi, lo), (hi, hi), (lo, lo)] + [(rng.integers(0, 256, d, dtype=np.uint8), rng.integers(0, 256, d, dtype=np.uint8)) for _ in range(6)]
    for x, q in pairs:
        want = int(((x.astype(np.int64) - q.astype(np.int64)) ** 2).sum())
        assert want < 1 << 24
        got = ku.f32_l2_four_sums(x, q)
        assert float(got) == want and ku.bits(got) == ku.bits(np.float32(want))
        if d % 8 == 0:
            dot = int((x.astype(np.int64) * q.astype(np.int64)).sum())
            assert dot < 1 << 24
            got = ku.f32_dot_eight_sums(x, q)
            assert float(got) == -dot
    assert int(((lo.astype(np.int64) - hi.astype(np.int64)) ** 2).sum()) == 65025 * d


def test_signed_shift_identities():
    """What the pack and the sweep rest on, in int32 as the kernels compute it: with x' = x - 128 (the byte with its top bit flipped, read
    as signed) L2 is unchanged and x.q = x'.q' + 128 (sum x' + sum q') + 16384 d."""
    for d in (8, 100, 256):
        x, q = ku.random_bytes(d, 40, d), ku.random_bytes(d + 1, 30, d)
        xs, qs = (x ^ 0x80).view(np.int8).astype(np.int32), (q ^ 0x80).view(np.int8).astype(np.int32)
        assert np.array_equal(xs, x.astype(np.int32) - 128)
        acc = qs @ xs.T
        l2 = (qs * qs).sum(1)[:, None] + (xs * xs).sum(1)[None, :] - 2 * acc
        if d % 4 == 0:
            assert np.array_equal(l2, ku.int_dist(x, q, ku.L2))
        dot = acc + np.int32(128) * (xs.sum(1, dtype=np.int32)[None, :] + qs.sum(1, dtype=np.int32)[:, None]) + np.int32(16384 * d)
        assert np.array_equal(-dot, ku.int_dist(x, q, ku.NEG_DOT)) and dot.dtype == np.int32

@pytest.mark.parametrize("metric,d", [(ku.L2, 30), (ku.L2, 256), (ku.NEG_DOT, 8), (ku.NEG_DOT, 256)])
def test_oracle_on_widened_bytes_equals_integer_knn(orc, metric, d):
    """The yardsticks of the GPU tests agree with each other: the oracle's restatement of the reference's float arithmetic on the widened
    arrays gives the integer (distance, id) order, ties and padding included."""
    base, q = ku.random_bytes(10 + d, 300, d), ku.random_bytes(11 + d, 20, d)
    q[0], q[1] = 255, 0
    base[5:20] //= 128    # a mass of ties among the near rows
    for k, n, so in ((7, 300, -1), (40, 300, 3), (12, 5, -1)):
        oi, od = orc.exact_knn(ku.widen(base[:n]), ku.widen(q), k, metric, self_offset=so, threads=2)
        wi, wd = ku.int_knn(base[:n], q, k, metric, self_offset=so)
        assert np.array_equal(oi, wi) and np.array_equal(ku.bits(od), ku.bits(wd)), (k, n, so)
