// The staging rules of the synthesis kernels (nearfield_simple.hip, nearfield_general.hip): how many distinct
// (ring, table cell) blocks a wave takes through LDS per ROUND, and in how many PASSES of order slots the wide
// ring instantiation takes a round's blocks through its buffer.  Constants and pure functions, so that the
// kernels, the launch code (nearfield.hip fill_nf_args) and the host - tools/synth_staging.cpp prints them, the
// census of tests/synth_cases.py reads them from there - share one statement of them.
#pragma once

#include "lens_pack.h"

namespace ml {

constexpr int SK_SLOTS = 6;                     // distinct (ring, cell) blocks staged per round, at most
// complex in the ring kernel's block buffer.  Twenty waves of a CU (five per SIMD) could have 8 KB each
// of its 160 KB - but at exactly that size a wave that ends leaves a hole only an identical neighbour
// fits and the measured occupancy drops by 6 %: a lens of narrow collections (up to SIMPLE_NARROW_SLOTS
// orders: six blocks at a fixed pitch) takes 6.2 KB, the wide instantiation ML_RING_LDS_WIDE complex
#ifndef ML_RING_LDS_WIDE
#define ML_RING_LDS_WIDE 448
#endif
// (narrow: six blocks of four orders, or EIGHT of three - the pitch is the lens' widest narrow collection's,
// NfArgs::narrow_pitch / narrow_cap: at NA 0.94 a patch spans five to six of the outer rings and more than one
// table cell, and every block beyond the round's capacity costs the wave a second round - the whole order loop
// again for a few lanes)
constexpr int SK_SLOTS_NARROW = 8;
constexpr int RING_LDS_NARROW = SK_SLOTS_NARROW * (3 * UNIT + 1), RING_LDS = ML_RING_LDS_WIDE;
static_assert(SK_SLOTS * (SIMPLE_NARROW_SLOTS * UNIT + 1) <= RING_LDS_NARROW, "six blocks of four orders fit");
// the narrow instantiation's pitch - complex between staged blocks: 16 x the orders of the lens' widest narrow
// collection (LensClass::narrow_slots_max), + 1 so that blocks start in different 16-byte bank slots - and the
// blocks per round that fit its buffer at that pitch: eight of up to three orders, six of four
constexpr int narrow_pitch(int narrow_slots_max) { return UNIT * narrow_slots_max + 1; }
constexpr int narrow_cap(int pitch) { return RING_LDS_NARROW / pitch < SK_SLOTS_NARROW ? RING_LDS_NARROW / pitch : SK_SLOTS_NARROW; }
static_assert(narrow_cap(narrow_pitch(3)) == SK_SLOTS_NARROW && narrow_cap(narrow_pitch(SIMPLE_NARROW_SLOTS)) == SK_SLOTS,
              "eight blocks of three orders, six of four");
// order slots per pass of the wide instantiation: what n blocks leave each other of the buffer,
// (RING_LDS / n - 1) / 16 for n = 1 ... 6 blocks, four bits each
constexpr unsigned slots_per_pass(int n) { return (unsigned)((RING_LDS / n - 1) / UNIT < 15 ? (RING_LDS / n - 1) / UNIT : 15); }
constexpr unsigned UPP_TABLE = slots_per_pass(1) | slots_per_pass(2) << 4 | slots_per_pass(3) << 8 | slots_per_pass(4) << 12 |
                               slots_per_pass(5) << 16 | slots_per_pass(6) << 20;
static_assert(slots_per_pass(SK_SLOTS) >= 1, "block buffer too small");
constexpr int SK_TYPES = 20;                    // centre: cell types per staged block (the reference's default K, lens_center.py:28)
static_assert(SK_TYPES == CENTER_GROUP, "the centre table's cell blocks hold groups of SK_TYPES types");

// the general kernel (nearfield_general.hip nearfield_field_kernel)
constexpr int NF_SLOTS = 6;                  // distinct (ring, cell) blocks staged per round
constexpr int NF_CHUNK = 4;                  // orders per staging pass (64 lanes = 4 x 4 x 4)

}  // namespace ml
