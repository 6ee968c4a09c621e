"""gd_prune_kernel at the edges of its wavefront and of its list capacity, on an MI355X (run with -m gpu): gbnns_build_graph_gd_device against
gbnns_build_graph_gd, bit for bit, reverse pass on and off.

One index of 1 200 x 32 full-mantissa rows (few nodes have two candidates at one float32 distance), candidate lists cut from an exact
1 100-NN table to lengths cycling through 0, 1, 63, 64, 65 (a wavefront's edge: the sort's smallest network), 1 023, 1 024 (the kernel's
capacity) and 1 025 (beyond it: the host), shuffled.  M = 2 (M / 2 = 1), 31 .. 33 and 63 / 64 (the kept list fills the wavefront: one kept
neighbour per lane) run on the device, M = 65 entirely on the host; M = 1 is outside both builders' contract (M >= 2) and both refuse it.
The nodes finished on the host are exactly the lists of 1 025 and the lists with two candidates at one distance -- a list of 1 024 adds
nothing.

On such rows the greedy pass keeps 5 .. 30 of a node's candidates (measured on the CPU), never a wavefront's worth.  So a second index,
`stars`: 8 hubs in 64 dimensions, each with 100 satellites at distinct radii along axes of their own (+-e_j, jittered in every coordinate):
a satellite is closer to its hub than to any other satellite, so the hub keeps candidates until it holds M -- its degree without the reverse
pass is exactly M for every M <= 64: lane M - 1 of the kept list is written, lane 63 at M = 64."""
import numpy as np
import pytest

import datagen

pytestmark = pytest.mark.gpu

N, D, K = 1200, 32, 1100
LENGTHS = (0, 1, 63, 64, 65, 1023, 1024, 1025)
DEVICE_MS = (2, 31, 32, 33, 63, 64)


@pytest.fixture(scope="module")
def g():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import gbnns_dim_red_amd as g
    g.load_library()  # raises if the HIP library was not built: no fallback
    return g


@pytest.fixture(scope="module")
def index(g):
    """x, the CSR lists, and per node: its list's length and whether two of its candidates (at a distance above the builder's 1e-10) share a
    float32 distance -- from the distances of the exact table, which are the builder's own arithmetic."""
    rng = np.random.Generator(np.random.PCG64(6400))
    x = datagen.full_mantissa(rng, N, D)
    knn, dist = g.exact_knn(x, x, K, self_offset=0, want_dist=True)
    assert (knn != 0xFFFFFFFF).all()
    length = np.array([LENGTHS[i % len(LENGTHS)] for i in range(N)])
    lists, tie = [], np.zeros(N, bool)
    for i in range(N):
        row = knn[i][:length[i]].copy()
        dd = dist[i][:length[i]]
        dd = dd[dd > np.float32(1e-10)]
        tie[i] = bool((dd[1:] == dd[:-1]).any())
        rng.shuffle(row)
        lists.append(row)
    koff, knbr = datagen.lists_to_csr(lists)
    assert np.array_equal(np.diff(koff.astype(np.int64)), length)
    return x, koff, knbr, length, tie


@pytest.fixture(scope="module")
def stars():
    """x [808 x 64], the CSR lists (a hub's: its 100 satellites; a satellite's: its hub and the other 99; shuffled), the hubs' rows."""
    rng = np.random.Generator(np.random.PCG64(6401))
    hubs, sats, d = 8, 100, 64
    rows, lists, hub_rows = [], [], []
    for h in range(hubs):
        centre = rng.standard_normal(d) * 50.0
        first = len(rows)
        hub_rows.append(first)
        rows.append(centre)
        radii = 1.0 + 0.01 * rng.permutation(sats)
        for j in range(sats):
            v = centre + rng.standard_normal(d) * 1e-3
            v[j % d] += radii[j] * (1.0 if j < d else -1.0)
            rows.append(v)
        members = np.arange(first, first + sats + 1)
        for i in members:
            row = members[members != i].astype(np.uint32)
            rng.shuffle(row)
            lists.append(row)
    koff, knbr = datagen.lists_to_csr(lists)
    return np.ascontiguousarray(np.array(rows), np.float32), koff, knbr, np.array(hub_rows)


@pytest.mark.parametrize("M", DEVICE_MS + (65,))
def test_the_kept_list_fills_the_wavefront(g, stars, M):
    x, koff, knbr, hubs = stars
    n = len(x)
    for rev in (True, False):
        w_off, w_nbr = g.build_graph_gd(koff, knbr, x, M, reverse=rev, threads=8)
        off, nbr, on_host = g.build_graph_gd_device(koff, knbr, x, M, reverse=rev, threads=8)
        assert np.array_equal(off, w_off) and np.array_equal(nbr, w_nbr), (M, rev)
        assert on_host == n if M > 64 else on_host < n // 2, (M, rev, on_host)
        if not rev:
            assert (np.diff(off.astype(np.int64))[hubs] == M).all(), (M, np.diff(off.astype(np.int64))[hubs])


@pytest.mark.parametrize("M", DEVICE_MS)
def test_device_pruning_at_the_wavefronts_edges(g, index, M):
    x, koff, knbr, length, tie = index
    host = int(((length > 1024) | tie).sum())
    assert int((length > 1024).sum()) == N // 8 and int(tie[length == 1024].sum()) < N // 16
    for rev in (True, False):
        w_off, w_nbr = g.build_graph_gd(koff, knbr, x, M, reverse=rev, threads=8)
        off, nbr, on_host = g.build_graph_gd_device(koff, knbr, x, M, reverse=rev, threads=8)
        print("gd edges", M, rev, "on host", on_host, "lists of 1 025:", N // 8, "lists with a tie:", int(tie.sum()))
        assert np.array_equal(off, w_off) and np.array_equal(nbr, w_nbr), (M, rev)
        assert on_host < N // 2, (M, rev, on_host)   # the device decided
        # the lists of 1 025 came back through the host; a list of 1 024 (or any other) only where two candidates tie
        assert on_host == host, (M, rev, on_host, host)


def test_m_65_is_all_host_and_m_1_is_refused(g, index):
    x, koff, knbr, length, tie = index
    for rev in (True, False):
        w_off, w_nbr = g.build_graph_gd(koff, knbr, x, 65, reverse=rev, threads=8)
        off, nbr, on_host = g.build_graph_gd_device(koff, knbr, x, 65, reverse=rev, threads=8)
        assert np.array_equal(off, w_off) and np.array_equal(nbr, w_nbr), rev
        assert on_host == N
    for build in (g.build_graph_gd, g.build_graph_gd_device):   # M >= 2 is both builders' contract (include/gbnns.h: GdParams M 2 .. 64)
        with pytest.raises(g.GbnnsError) as e:
            build(koff, knbr, x, 1, threads=8)
        assert e.value.code == 1
