// launch_util.h -- host-side helpers shared by the kernel families' launchers: the LDS attribute, and the instance tables of the walk units (separate
// units so that the instantiations build in parallel; which of them serves a shape is plan_walk's business -- walk_plan.cpp -- not theirs).
#pragma once

#include "walk_plan.h"

namespace gbnns {

template <typename K>
static hipError_t set_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024)
        return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    return hipSuccess;
}

// One row of a unit's instance table: the instance (walk_plan.h), its kernel, and the kernel's printable name -- taken from the same
// expression as the pointer, written with every template argument the way the demangler prints it.
struct WalkEntry {
    WalkInstance inst;
    const void* fn;
    const char* name;
};
#define WALK_KERNEL(...) reinterpret_cast<const void*>(&__VA_ARGS__), #__VA_ARGS__
// (macro arguments: the kernel's own template arguments, which its printable name needs as written; the row's flags are built from them by name
// -- for the register-list / two-list kernels by reg_flags, walk_generic.h, the expression the kernel itself hands to its walk)
#define WALK_REG(M, S, OFF32, RETRY, R, ONE, AUX) {{WalkFamily::RegList, M, S, R, reg_flags(OFF32, RETRY, ONE, AUX)}, WALK_KERNEL(walk_reg_kernel<M, S, OFF32, RETRY, R, ONE, AUX>)}
#define WALK_BIG(M, S, OFF32, RETRY, AUX, ONE, LATE) {{WalkFamily::TwoList, M, S, 4, reg_flags(OFF32, RETRY, ONE, AUX, LATE)}, WALK_KERNEL(walk_reg_big_kernel<M, S, OFF32, RETRY, AUX, ONE, LATE>)}
#define WALK_LDS(M, S, RETRY, PACKED) {{WalkFamily::LdsList, M, S, 0, flag_if(RETRY, kRetry) | flag_if(PACKED, kPacked)}, WALK_KERNEL(walk_fast_kernel<M, S, RETRY, PACKED>)}
#define WALK_WIDE(S, LATE) {{WalkFamily::RegWide, 0, S, 0, flag_if(LATE, kLate)}, WALK_KERNEL(walk_reg_wide_kernel<S, LATE>)}
// per (metric, steps): the LDS-list kernels; R list registers, and the two-list kernels (+ first pass over one-pass adjacency rows): compact /
// non-compact index x first pass / retry, the auxiliary-graph hop
#define WALK_LDS_SET(M, S) WALK_LDS(M, S, false, false), WALK_LDS(M, S, false, true), WALK_LDS(M, S, true, false), WALK_LDS(M, S, true, true)
#define WALK_REG_SET(M, S, R)                                                                                                       \
    WALK_REG(M, S, true, false, R, false, false), WALK_REG(M, S, true, true, R, false, false), WALK_REG(M, S, false, false, R, false, false), \
        WALK_REG(M, S, false, true, R, false, false), WALK_REG(M, S, true, false, R, false, true), WALK_REG(M, S, true, true, R, false, true)
#define WALK_BIG_SET(M, S)                                                                                                                   \
    WALK_BIG(M, S, true, false, false, false, false), WALK_BIG(M, S, true, true, false, false, false), WALK_BIG(M, S, false, false, false, false, false), \
        WALK_BIG(M, S, false, true, false, false, false), WALK_BIG(M, S, true, false, true, false, false), WALK_BIG(M, S, true, true, true, false, false), \
        WALK_BIG(M, S, true, false, false, true, false)
// ef <= 64: one list register per lane (+ the loop-free expansion over one-pass adjacency rows); ef <= 128: two; beyond that the two-list
// kernels; ef > 1 024 (and auxiliary-graph walks over a non-compact index): the list lives in LDS
#define WALK_GENERIC_SET(M, S) WALK_LDS_SET(M, S), WALK_REG_SET(M, S, 1), WALK_REG(M, S, true, false, 1, true, false), WALK_REG_SET(M, S, 2), WALK_BIG_SET(M, S)
// (the rows requested after the visited test: one- and two-pass adjacency rows)
#define WALK_BIG_LATE(S) WALK_BIG(0, S, true, false, false, true, true), WALK_BIG(0, S, true, false, false, false, true)

template <size_t N> static const WalkEntry* find_walk_entry(const WalkEntry (&rows)[N], const WalkInstance& k) {
    for (const WalkEntry& r : rows)
        if (r.inst == k) return &r;
    return nullptr;
}

// The units' tables: the entry of an instance, nullptr when the unit does not hold it.  walk_entry (walk_l2.hip) asks them all.
const WalkEntry* walk_l2_entry(const WalkInstance& k);
const WalkEntry* walk_dot_entry(const WalkInstance& k);
const WalkEntry* walk_wide_entry(const WalkInstance& k);
const WalkEntry* walk_wide2_entry(const WalkInstance& k);
const WalkEntry* walk_wide3_entry(const WalkInstance& k);
const WalkEntry* walk_hot_entry(const WalkInstance& k);
const WalkEntry* walk_coop_entry(const WalkInstance& k);
const WalkEntry* walk_bitmap_entry(const WalkInstance& k);
const WalkEntry* walk_half_entry(const WalkInstance& k);
// (tables of their own, asked last by walk_entry, walk_l2.hip: only an instance with kTag / kBridge / kByteWalk / kByteQuery / kHalfWalk set matches a row of them)
const WalkEntry* walk_tag_entry(const WalkInstance& k);
const WalkEntry* walk_bridge_entry(const WalkInstance& k);
const WalkEntry* walk_bytes_entry(const WalkInstance& k);
const WalkEntry* walk_bytes_q_entry(const WalkInstance& k);
const WalkEntry* walk_half_base_entry(const WalkInstance& k);

}  // namespace gbnns
