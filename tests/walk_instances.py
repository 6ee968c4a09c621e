"""The census of the walk kernel instances: one static table of search cases that, between them, launch every one of the 210
instances of the first, the bitmap and the retry pass (tests/golden/walk_launches_before_plan.tsv.gz lists them), and the data those
cases run on.  A plain module: tests/test_cabi_cpu.py proves on the CPU that the table covers the 210 names exactly and that every retry
case's walks outgrow its visited set; tests/test_gpu_walk_instances.py runs every case on the device, bit-exact against the oracle,
and asserts the launched names.

A case is what a caller can set -- metric, walked dimension, the graph's degree class, the auxiliary graph, the beam, GBNNS_FLAG_WIDE_INDEX /
GBNNS_FLAG_BITMAP_PASS, the handle knobs, hash_capacity -- plus the names that must come out: `first` (first or bitmap pass) and, for
hash_capacity != 0, `retry`.  The table was chosen so that the names cover the golden file (retry cases first: they name two
instances each), then filled up with ef = 1 and ef = 8 on every first-pass family that serves short lists, one padded dimension (30:
dim != row stride) at one beam per family, and beams on either side of the list-length boundaries 64 / 128 / 200 / 1 024.  Retry cases
use the longest beam of their class (64, 128, 200, 1 100; 1 024 for the 512-byte pair form, which only serves beams beyond 200) and
never one below 64: their walks have to outgrow a 128-entry visited set (at ef >= 64 every query computes several hundred distances).
"""
import collections
import functools

import numpy as np

import datagen

NQ = 96                  # queries per case
D_ORIG = 40              # original space of the MODE_LOWQ searches: d % 8 == 0, so every instance that fuses the re-rank runs it
ELL_STRIDE = {30: 32, 60: 64, 90: 96}    # degree class (largest degree of random_graph(rng, n, 2, deg)) -> adjacency stride in slots
AUX_STRIDE = 16          # random_graph(rng, n, 0, 6)
FLAG_WIDE_INDEX, FLAG_BITMAP_PASS = 16, 32   # include/gbnns.h
BEAMS = (1, 8, 64, 65, 128, 129, 200, 201, 512, 1024, 1100)
DIMS = (30, 32, 40, 48, 64, 96, 128, 144)


class Case(collections.namedtuple("Case", "metric dim deg aux ef wide bitmap coop late_rows spec hash_capacity first retry")):
    __slots__ = ()

    @property
    def n(self):
        """Rows of the index: 6 000 beyond the register lists, so that the walk does not exhaust the graph."""
        return 6000 if self.ef > 1024 else 3000

    @property
    def knobs(self):
        """The handle knobs of the case.  spec: the ef <= 64 hot instance requests a hop's rows before its visited test whatever the
        batch size and the visited set's form; spec_tail 0: no wavefront does so by its place in the launch."""
        return {"coop": self.coop, "late_rows": self.late_rows, "spec_min_nq": 1 if self.spec else 0, "spec_any_form": self.spec, "spec_tail": 0}

    @property
    def flags(self):
        return (FLAG_WIDE_INDEX if self.wide else 0) | (FLAG_BITMAP_PASS if self.bitmap else 0)

    @property
    def first_pass(self):
        return 1 if self.bitmap else 0   # gbnns_debug_walk_plan's pass number

    def plan_args(self, pas):
        """Arguments of gbnns_debug_walk_plan (up to rr_reserve) for pass `pas` with the decisions a search of this case resolves: the
        knobs are explicit (never -1), the two-wavefront walk is not asked for with either flag, one entry point per query."""
        return (self.metric, self.dim, (self.dim + 3) // 4 * 4, self.n, ELL_STRIDE[self.deg], AUX_STRIDE if self.aux else 0, self.ef, 1, self.wide,
                int(self.coop and not self.bitmap and not self.wide), self.late_rows, self.spec, pas, 4 * D_ORIG)

    @property
    def graph_key(self):
        return (self.metric, self.dim, self.n, self.deg)


# metric, dim, deg, aux, ef, wide, bitmap, coop, late_rows, spec, hash_capacity, first / bitmap pass, retry pass
_TABLE = [
    (0,  32, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_hot_kernel",                                                     None),
    (0,  32, 30, 0,    1, 0, 0, 0, 0, 1,   0, "walk_hot_spec_kernel",                                                None),
    (0,  32, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_hot_kernel",                                                     None),
    (0,  32, 30, 0,    8, 0, 0, 0, 0, 1,   0, "walk_hot_spec_kernel",                                                None),
    (0,  32, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_hot_kernel",                                                     None),
    (0,  32, 30, 0,   65, 0, 0, 0, 0, 0,   0, "walk_hot2_kernel",                                                    None),
    (0,  32, 30, 0,  128, 0, 0, 0, 0, 0,   0, "walk_hot2_kernel",                                                    None),
    (0,  32, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_hot_big_kernel",                                                 None),
    (0,  32, 30, 0,  200, 0, 0, 1, 0, 0,   0, "walk_coop_kernel<8, false>",                                          None),
    (0,  32, 30, 0,  200, 0, 0, 1, 1, 0,   0, "walk_coop_kernel<8, true>",                                           None),
    (0,  32, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_hot_big_kernel",                                                 None),
    (0,  32, 30, 0, 1024, 0, 0, 0, 0, 0,   0, "walk_hot_big_kernel",                                                 None),
    (0,  32, 30, 0,    1, 0, 1, 0, 0, 0,   0, "walk_bitmap_reg_kernel<0, 1>",                                        None),
    (0,  32, 30, 0,    8, 0, 1, 0, 0, 0,   0, "walk_bitmap_reg_kernel<0, 1>",                                        None),
    (0,  32, 30, 0,  128, 0, 1, 0, 0, 0,   0, "walk_bitmap_reg_kernel<0, 2>",                                        None),
    (0,  32, 30, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<0, 8, true, false>",                           None),
    (0,  32, 30, 0, 1100, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<0, 8>",                                            None),
    (0,  32, 30, 1,    1, 1, 0, 0, 0, 0,   0, "walk_fast_kernel<0, 8, false, false>",                                None),
    (0,  32, 30, 1,    8, 1, 0, 0, 0, 0,   0, "walk_fast_kernel<0, 8, false, false>",                                None),
    (0,  32, 60, 0,    1, 0, 0, 0, 0, 0,   0, "walk_hotw_kernel",                                                    None),
    (0,  32, 60, 0,    8, 0, 0, 0, 0, 0,   0, "walk_hotw_kernel",                                                    None),
    (0,  32, 60, 0,  128, 0, 0, 0, 0, 0,   0, "walk_hotw2_kernel",                                                   None),
    (0,  32, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_hotw_big_kernel",                                                None),
    (0,  32, 60, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<0, 8, false, false>",                          None),
    (0,  32, 90, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 8, true, false, 1, false, false>",                 None),
    (0,  32, 90, 0,  128, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 8, true, false, 2, false, false>",                 None),
    (0,  32, 90, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 8, true, false, false, false, false>",         None),
    (0,  32, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_hot_kernel",                                                     "walk_reg_kernel<0, 8, true, true, 1, false, false>"),
    (0,  32, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_hot2_kernel",                                                    "walk_reg_kernel<0, 8, true, true, 2, false, false>"),
    (0,  32, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_hot_big_kernel",                                                 "walk_reg_big_kernel<0, 8, true, true, false, false, false>"),
    (0,  32, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 8, false, true>",                                 "walk_fast_kernel<0, 8, true, true>"),
    (0,  32, 30, 0,   64, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 8, false, false, 1, false, false>",                "walk_reg_kernel<0, 8, false, true, 1, false, false>"),
    (0,  32, 30, 0,  128, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 8, false, false, 2, false, false>",                "walk_reg_kernel<0, 8, false, true, 2, false, false>"),
    (0,  32, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 8, false, false, false, false, false>",        "walk_reg_big_kernel<0, 8, false, true, false, false, false>"),
    (0,  32, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 8, false, false>",                                "walk_fast_kernel<0, 8, true, false>"),
    (0,  32, 30, 1,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 8, true, false, 1, false, true>",                  "walk_reg_kernel<0, 8, true, true, 1, false, true>"),
    (0,  32, 30, 1,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 8, true, false, 2, false, true>",                  "walk_reg_kernel<0, 8, true, true, 2, false, true>"),
    (0,  32, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 8, true, false, true, false, false>",          "walk_reg_big_kernel<0, 8, true, true, true, false, false>"),
    (0,  40, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0,  40, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0,  40, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0,  40, 30, 0,   65, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 2, false, false>",                 None),
    (0,  40, 30, 0,  128, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 2, false, false>",                 None),
    (0,  40, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  40, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  40, 30, 0,  201, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  40, 30, 0,  512, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  40, 30, 0, 1024, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  40, 30, 0, 1100, 0, 0, 0, 0, 0,   0, "walk_fast_kernel<0, 0, false, true>",                                 None),
    (0,  40, 60, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0,  40, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  40, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  "walk_reg_kernel<0, 0, true, true, 1, false, false>"),
    (0,  40, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 0, true, false, 2, false, false>",                 "walk_reg_kernel<0, 0, true, true, 2, false, false>"),
    (0,  40, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          "walk_reg_big_kernel<0, 0, true, true, false, false, false>"),
    (0,  40, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 0, false, true>",                                 "walk_fast_kernel<0, 0, true, true>"),
    (0,  48, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_wide_kernel<12, false>",                                     None),
    (0,  48, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_wide_kernel<12, false>",                                     None),
    (0,  48, 30, 0,   64, 0, 0, 0, 1, 0,   0, "walk_reg_wide_kernel<12, true>",                                      None),
    (0,  48, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 12, true, false, false, true, false>",         None),
    (0,  48, 30, 0,  200, 0, 0, 1, 0, 0,   0, "walk_coop_kernel<12, false>",                                         None),
    (0,  48, 30, 0,  200, 0, 0, 1, 1, 0,   0, "walk_coop_kernel<12, true>",                                          None),
    (0,  48, 30, 0,    1, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<0, 0>",                                            None),
    (0,  48, 30, 0,    8, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<0, 0>",                                            None),
    (0,  48, 60, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 12, true, false, 1, false, false>",                None),
    (0,  48, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 12, true, false, false, false, false>",        None),
    (0,  48, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_reg_wide_kernel<12, false>",                                     "walk_reg_kernel<0, 12, true, true, 1, false, false>"),
    (0,  48, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 12, true, false, 2, false, false>",                "walk_reg_kernel<0, 12, true, true, 2, false, false>"),
    (0,  48, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 12, true, false, false, true, false>",         "walk_reg_big_kernel<0, 12, true, true, false, false, false>"),
    (0,  48, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 12, false, true>",                                "walk_fast_kernel<0, 12, true, true>"),
    (0,  48, 30, 0,   64, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 12, false, false, 1, false, false>",               "walk_reg_kernel<0, 12, false, true, 1, false, false>"),
    (0,  48, 30, 0,  128, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 12, false, false, 2, false, false>",               "walk_reg_kernel<0, 12, false, true, 2, false, false>"),
    (0,  48, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 12, false, false, false, false, false>",       "walk_reg_big_kernel<0, 12, false, true, false, false, false>"),
    (0,  48, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 12, false, false>",                               "walk_fast_kernel<0, 12, true, false>"),
    (0,  48, 30, 1,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 12, true, false, 1, false, true>",                 "walk_reg_kernel<0, 12, true, true, 1, false, true>"),
    (0,  48, 30, 1,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 12, true, false, 2, false, true>",                 "walk_reg_kernel<0, 12, true, true, 2, false, true>"),
    (0,  48, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 12, true, false, true, false, false>",         "walk_reg_big_kernel<0, 12, true, true, true, false, false>"),
    (0,  64, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_wide_kernel<16, false>",                                     None),
    (0,  64, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_wide_kernel<16, false>",                                     None),
    (0,  64, 30, 0,   64, 0, 0, 0, 1, 0,   0, "walk_reg_wide_kernel<16, true>",                                      None),
    (0,  64, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_wide_kernel<16, false>",                                     None),
    (0,  64, 30, 0,  200, 0, 0, 1, 0, 0,   0, "walk_coop_kernel<16, false>",                                         None),
    (0,  64, 30, 0,  200, 0, 0, 1, 1, 0,   0, "walk_coop_kernel<16, true>",                                          None),
    (0,  64, 30, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<0, 16, true, false>",                          None),
    (0,  64, 60, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 16, true, false, 1, false, false>",                None),
    (0,  64, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 16, true, false, false, false, false>",        None),
    (0,  64, 60, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<0, 16, false, false>",                         None),
    (0,  64, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_reg_wide_kernel<16, false>",                                     "walk_reg_kernel<0, 16, true, true, 1, false, false>"),
    (0,  64, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 16, true, false, 2, false, false>",                "walk_reg_kernel<0, 16, true, true, 2, false, false>"),
    (0,  64, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 16, true, false, false, true, false>",         "walk_reg_big_kernel<0, 16, true, true, false, false, false>"),
    (0,  64, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 16, false, true>",                                "walk_fast_kernel<0, 16, true, true>"),
    (0,  64, 30, 0,   64, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 16, false, false, 1, false, false>",               "walk_reg_kernel<0, 16, false, true, 1, false, false>"),
    (0,  64, 30, 0,  128, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 16, false, false, 2, false, false>",               "walk_reg_kernel<0, 16, false, true, 2, false, false>"),
    (0,  64, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 16, false, false, false, false, false>",       "walk_reg_big_kernel<0, 16, false, true, false, false, false>"),
    (0,  64, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 16, false, false>",                               "walk_fast_kernel<0, 16, true, false>"),
    (0,  64, 30, 1,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 16, true, false, 1, false, true>",                 "walk_reg_kernel<0, 16, true, true, 1, false, true>"),
    (0,  64, 30, 1,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 16, true, false, 2, false, true>",                 "walk_reg_kernel<0, 16, true, true, 2, false, true>"),
    (0,  64, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 16, true, false, true, false, false>",         "walk_reg_big_kernel<0, 16, true, true, true, false, false>"),
    (0,  96, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 24, true, false, 1, true, false>",                 None),
    (0,  96, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 24, true, false, 1, true, false>",                 None),
    (0,  96, 30, 0,   65, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 24, true, false, 2, true, false>",                 None),
    (0,  96, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 24, true, false, false, true, false>",         None),
    (0,  96, 30, 0,  200, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 24, true, false, false, true, true>",          None),
    (0,  96, 30, 0, 1024, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 24, true, false, false, true, false>",         None),
    (0,  96, 60, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 24, true, false, 1, false, false>",                None),
    (0,  96, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 24, true, false, false, false, false>",        None),
    (0,  96, 60, 0,  200, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 24, true, false, false, false, true>",         None),
    (0,  96, 90, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, false, false>",                 None),
    (0,  96, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 24, true, false, 1, true, false>",                 "walk_reg_kernel<0, 0, true, true, 1, false, false>"),
    (0,  96, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 24, true, false, 2, true, false>",                 "walk_reg_kernel<0, 0, true, true, 2, false, false>"),
    (0,  96, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 24, true, false, false, true, false>",         "walk_reg_big_kernel<0, 24, true, true, false, false, false>"),
    (0,  96, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 0, false, true>",                                 "walk_fast_kernel<0, 0, true, true>"),
    (0,  96, 30, 0,   64, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 0, false, false, 1, false, false>",                "walk_reg_kernel<0, 0, false, true, 1, false, false>"),
    (0,  96, 30, 0,  128, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 0, false, false, 2, false, false>",                "walk_reg_kernel<0, 0, false, true, 2, false, false>"),
    (0,  96, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 24, false, false, false, false, false>",       "walk_reg_big_kernel<0, 24, false, true, false, false, false>"),
    (0,  96, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 0, false, false>",                                "walk_fast_kernel<0, 0, true, false>"),
    (0,  96, 30, 1,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 0, true, false, 1, false, true>",                  "walk_reg_kernel<0, 0, true, true, 1, false, true>"),
    (0,  96, 30, 1,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<0, 0, true, false, 2, false, true>",                  "walk_reg_kernel<0, 0, true, true, 2, false, true>"),
    (0,  96, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 24, true, false, true, false, false>",         "walk_reg_big_kernel<0, 24, true, true, true, false, false>"),
    (0, 128, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0, 128, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0, 128, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0, 128, 30, 0,  128, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 2, false, false>",                 None),
    (0, 128, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0, 128, 30, 0,  201, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 32, true, false, false, true, false>",         None),
    (0, 128, 30, 0,  512, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 32, true, false, false, true, true>",          None),
    (0, 128, 60, 0,  512, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 32, true, false, false, false, false>",        None),
    (0, 128, 60, 0,  512, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 32, true, false, false, false, true>",         None),
    (0, 128, 90, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, false, false>",         None),
    (0, 128, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          "walk_reg_big_kernel<0, 0, true, true, false, false, false>"),
    (0, 128, 30, 0, 1024, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 32, true, false, false, true, false>",         "walk_reg_big_kernel<0, 32, true, true, false, false, false>"),
    (0, 128, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 0, false, false, false, false, false>",        "walk_reg_big_kernel<0, 0, false, true, false, false, false>"),
    (0, 128, 30, 0, 1024, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 32, false, false, false, false, false>",       "walk_reg_big_kernel<0, 32, false, true, false, false, false>"),
    (0, 128, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 0, true, false, true, false, false>",          "walk_reg_big_kernel<0, 0, true, true, true, false, false>"),
    (0, 128, 30, 1, 1024, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 32, true, false, true, false, false>",         "walk_reg_big_kernel<0, 32, true, true, true, false, false>"),
    (0, 144, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0, 144, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0, 144, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0, 144, 30, 0,  128, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 2, false, false>",                 None),
    (0, 144, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, true, false>",         None),
    (0, 144, 30, 0,  200, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, true, true>",          None),
    (0, 144, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, true, false>",         None),
    (0, 144, 30, 0,  512, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, true, false>",         None),
    (0, 144, 30, 0, 1024, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, true, false>",         None),
    (0, 144, 30, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<0, 36, true, false>",                          None),
    (0, 144, 30, 0,  200, 0, 1, 0, 1, 0,   0, "walk_bitmap_big_kernel<0, 36, true, true>",                           None),
    (0, 144, 30, 0,  512, 0, 1, 0, 1, 0,   0, "walk_bitmap_big_kernel<0, 36, true, true>",                           None),
    (0, 144, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, false, false>",        None),
    (0, 144, 60, 0,  200, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, false, true>",         None),
    (0, 144, 60, 0,  512, 0, 0, 0, 1, 0,   0, "walk_reg_big_kernel<0, 36, true, false, false, false, true>",         None),
    (0, 144, 60, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<0, 36, false, false>",                         None),
    (0, 144, 60, 0,  200, 0, 1, 0, 1, 0,   0, "walk_bitmap_big_kernel<0, 36, false, true>",                          None),
    (0, 144, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 36, true, false, false, true, false>",         "walk_reg_big_kernel<0, 36, true, true, false, false, false>"),
    (0, 144, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 36, false, true>",                                "walk_fast_kernel<0, 36, true, true>"),
    (0, 144, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 36, false, false, false, false, false>",       "walk_reg_big_kernel<0, 36, false, true, false, false, false>"),
    (0, 144, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<0, 36, false, false>",                               "walk_fast_kernel<0, 36, true, false>"),
    (0, 144, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<0, 36, true, false, true, false, false>",         "walk_reg_big_kernel<0, 36, true, true, true, false, false>"),
    (0,  30, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<0, 0, true, false, 1, true, false>",                  None),
    (0,  30, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<0, 0, true, false, false, true, false>",          None),
    (0,  30, 30, 0, 1100, 0, 0, 0, 0, 0,   0, "walk_fast_kernel<0, 0, false, true>",                                 None),
    (0,  30, 30, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<0, 0>",                                            None),
    (1,  32, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<1, false>",                                       None),
    (1,  32, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<1, false>",                                       None),
    (1,  32, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<1, false>",                                       None),
    (1,  32, 30, 0,   65, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<2, false>",                                       None),
    (1,  32, 30, 0,  128, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<2, false>",                                       None),
    (1,  32, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_hot_dot_big_kernel<false>",                                      None),
    (1,  32, 30, 0,  512, 0, 0, 0, 0, 0,   0, "walk_hot_dot_big_kernel<false>",                                      None),
    (1,  32, 30, 0,    1, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<1, 0>",                                            None),
    (1,  32, 30, 0,    8, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<1, 0>",                                            None),
    (1,  32, 30, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<1, 8, true, false>",                           None),
    (1,  32, 30, 1,    1, 1, 0, 0, 0, 0,   0, "walk_fast_kernel<1, 8, false, false>",                                None),
    (1,  32, 30, 1,    8, 1, 0, 0, 0, 0,   0, "walk_fast_kernel<1, 8, false, false>",                                None),
    (1,  32, 60, 0,   64, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<1, true>",                                        None),
    (1,  32, 60, 0,  128, 0, 0, 0, 0, 0,   0, "walk_hot_dot_kernel<2, true>",                                        None),
    (1,  32, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_hot_dot_big_kernel<true>",                                       None),
    (1,  32, 60, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_big_kernel<1, 8, false, false>",                          None),
    (1,  32, 90, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 8, true, false, 1, false, false>",                 None),
    (1,  32, 90, 0,  128, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 8, true, false, 2, false, false>",                 None),
    (1,  32, 90, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 8, true, false, false, false, false>",         None),
    (1,  32, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_hot_dot_kernel<1, false>",                                       "walk_reg_kernel<1, 8, true, true, 1, false, false>"),
    (1,  32, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_hot_dot_kernel<2, false>",                                       "walk_reg_kernel<1, 8, true, true, 2, false, false>"),
    (1,  32, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_hot_dot_big_kernel<false>",                                      "walk_reg_big_kernel<1, 8, true, true, false, false, false>"),
    (1,  32, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<1, 8, false, true>",                                 "walk_fast_kernel<1, 8, true, true>"),
    (1,  32, 30, 0,   64, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 8, false, false, 1, false, false>",                "walk_reg_kernel<1, 8, false, true, 1, false, false>"),
    (1,  32, 30, 0,  128, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 8, false, false, 2, false, false>",                "walk_reg_kernel<1, 8, false, true, 2, false, false>"),
    (1,  32, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<1, 8, false, false, false, false, false>",        "walk_reg_big_kernel<1, 8, false, true, false, false, false>"),
    (1,  32, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<1, 8, false, false>",                                "walk_fast_kernel<1, 8, true, false>"),
    (1,  32, 30, 1,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 8, true, false, 1, false, true>",                  "walk_reg_kernel<1, 8, true, true, 1, false, true>"),
    (1,  32, 30, 1,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 8, true, false, 2, false, true>",                  "walk_reg_kernel<1, 8, true, true, 2, false, true>"),
    (1,  32, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<1, 8, true, false, true, false, false>",          "walk_reg_big_kernel<1, 8, true, true, true, false, false>"),
    (1,  40, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  None),
    (1,  40, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  None),
    (1,  40, 30, 0,   65, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 2, false, false>",                 None),
    (1,  40, 30, 0,  129, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1,  40, 30, 0,  201, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1,  40, 30, 0,  512, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1,  40, 30, 0, 1024, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1,  40, 90, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, false, false>",                 None),
    (1,  40, 90, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, false, false>",         None),
    (1,  40, 30, 0,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  "walk_reg_kernel<1, 0, true, true, 1, false, false>"),
    (1,  40, 30, 0,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 0, true, false, 2, false, false>",                 "walk_reg_kernel<1, 0, true, true, 2, false, false>"),
    (1,  40, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          "walk_reg_big_kernel<1, 0, true, true, false, false, false>"),
    (1,  40, 30, 0, 1100, 0, 0, 0, 0, 0, 128, "walk_fast_kernel<1, 0, false, true>",                                 "walk_fast_kernel<1, 0, true, true>"),
    (1,  40, 30, 0,   64, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 0, false, false, 1, false, false>",                "walk_reg_kernel<1, 0, false, true, 1, false, false>"),
    (1,  40, 30, 0,  128, 1, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 0, false, false, 2, false, false>",                "walk_reg_kernel<1, 0, false, true, 2, false, false>"),
    (1,  40, 30, 0,  200, 1, 0, 0, 0, 0, 128, "walk_reg_big_kernel<1, 0, false, false, false, false, false>",        "walk_reg_big_kernel<1, 0, false, true, false, false, false>"),
    (1,  40, 30, 0, 1100, 1, 0, 0, 0, 0, 128, "walk_fast_kernel<1, 0, false, false>",                                "walk_fast_kernel<1, 0, true, false>"),
    (1,  40, 30, 1,   64, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 0, true, false, 1, false, true>",                  "walk_reg_kernel<1, 0, true, true, 1, false, true>"),
    (1,  40, 30, 1,  128, 0, 0, 0, 0, 0, 128, "walk_reg_kernel<1, 0, true, false, 2, false, true>",                  "walk_reg_kernel<1, 0, true, true, 2, false, true>"),
    (1,  40, 30, 1,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<1, 0, true, false, true, false, false>",          "walk_reg_big_kernel<1, 0, true, true, true, false, false>"),
    (1, 144, 30, 0,    1, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  None),
    (1, 144, 30, 0,    8, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  None),
    (1, 144, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  None),
    (1, 144, 30, 0,  128, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 2, false, false>",                 None),
    (1, 144, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1, 144, 30, 0,  512, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1, 144, 30, 0, 1100, 0, 0, 0, 0, 0,   0, "walk_fast_kernel<1, 0, false, true>",                                 None),
    (1, 144, 60, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1, 144, 30, 0,  200, 0, 0, 0, 0, 0, 128, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          "walk_reg_big_kernel<1, 0, true, true, false, false, false>"),
    (1,  30, 30, 0,   64, 0, 0, 0, 0, 0,   0, "walk_reg_kernel<1, 0, true, false, 1, true, false>",                  None),
    (1,  30, 30, 0,  200, 0, 0, 0, 0, 0,   0, "walk_reg_big_kernel<1, 0, true, false, false, true, false>",          None),
    (1,  30, 30, 0, 1100, 0, 0, 0, 0, 0,   0, "walk_fast_kernel<1, 0, false, true>",                                 None),
    (1,  30, 30, 0,  200, 0, 1, 0, 0, 0,   0, "walk_bitmap_kernel<1, 0>",                                            None),
]
CASES = [Case(*row) for row in _TABLE]
SETS = sorted({(c.metric, c.dim) for c in CASES})   # one parameter set of the device census each


def _rng(*key):
    return np.random.Generator(np.random.PCG64(list((7100,) + key)))


@functools.lru_cache(maxsize=None)
def vectors(metric, dim, n):
    """Full-mantissa walked rows [n x dim] and queries [NQ x dim], independent full-mantissa original-space rows [n x D_ORIG] and
    queries, random entry ids.  Treat as read-only: shared by every case of the set."""
    rng = _rng(metric, dim, n)
    return dict(db_low=datagen.full_mantissa(rng, n, dim), q_low=datagen.full_mantissa(rng, NQ, dim),
                base=datagen.full_mantissa(rng, n, D_ORIG), queries=datagen.full_mantissa(rng, NQ, D_ORIG),
                ent=rng.integers(0, n, size=NQ).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def graph(metric, dim, n, deg):
    return datagen.random_graph(_rng(metric, dim, n, deg), n, 2, deg)


@functools.lru_cache(maxsize=None)
def aux_graph(metric, dim, n):
    return datagen.random_graph(_rng(metric, dim, n, 6), n, 0, 6)


_WALKS = {}


def oracle_walk(orc, case):
    """(walk, re-ranked answers) of the oracle on the case's data, computed once per (data, graph, auxiliary graph, beam): neither the
    flags, nor the knobs, nor the visited set's size may change a result."""
    key = case.graph_key + (case.aux, case.ef)
    if key not in _WALKS:
        v = vectors(case.metric, case.dim, case.n)
        off, nbr = graph(*case.graph_key)
        kw = dict(aux=aux_graph(case.metric, case.dim, case.n), llf=True, hops_bound=50) if case.aux else {}
        w = orc.walk(v["q_low"], v["db_low"], off, nbr, case.ef, entries=v["ent"], metric=case.metric, threads=8, **kw)
        _WALKS[key] = (w, orc.rerank(v["queries"], w["ids"], w["count"], v["base"], metric=case.metric, threads=8))
    return _WALKS[key]
