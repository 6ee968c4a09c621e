// walk_bitmap.hip -- the first pass with the visited sets as bitmaps in HBM (large ef on deep batches): persistent
// wavefronts, one bitmap slot each.
#include "launch_util.h"
#include "walk_generic.h"

namespace gbnns {

// Register lists (ef <= 128, L2, 128-byte rows); the two-list walk over 128-byte rows (both metrics) and, pair form with L2, 256- and
// 576-byte rows -- adjacency rows of one 32-slot pass, the common case, take the instance without the pass loop, 576-byte rows have
// the rows-after-the-bit-test order too; the LDS-list walk for everything else.
#define WALK_BITMAP_BIG(M, S, ONE, LATE) {{WalkFamily::BitmapBig, M, S, 0, flag_if(ONE, kOne) | flag_if(LATE, kLate)}, WALK_KERNEL(walk_bitmap_big_kernel<M, S, ONE, LATE>)}
#define WALK_BITMAP_LDS(M, S) {{WalkFamily::BitmapLds, M, S}, WALK_KERNEL(walk_bitmap_kernel<M, S>)}
static const WalkEntry kEntries[] = {
    {{WalkFamily::BitmapReg, 0, 0, 1}, WALK_KERNEL(walk_bitmap_reg_kernel<0, 1>)},
    {{WalkFamily::BitmapReg, 0, 0, 2}, WALK_KERNEL(walk_bitmap_reg_kernel<0, 2>)},
    WALK_BITMAP_BIG(0, 8, true, false), WALK_BITMAP_BIG(0, 8, false, false), WALK_BITMAP_BIG(1, 8, true, false), WALK_BITMAP_BIG(1, 8, false, false),
    WALK_BITMAP_BIG(0, 16, true, false), WALK_BITMAP_BIG(0, 16, false, false),
    WALK_BITMAP_BIG(0, 36, true, false), WALK_BITMAP_BIG(0, 36, false, false), WALK_BITMAP_BIG(0, 36, true, true), WALK_BITMAP_BIG(0, 36, false, true),
    WALK_BITMAP_LDS(0, 0), WALK_BITMAP_LDS(0, 8), WALK_BITMAP_LDS(1, 0),
};
const WalkEntry* walk_bitmap_entry(const WalkInstance& k) { return find_walk_entry(kEntries, k); }

}  // namespace gbnns
