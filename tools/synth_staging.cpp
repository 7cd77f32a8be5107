// Prints the staging rules of the synthesis kernels (metalens_amd/csrc/synth_staging.h): what the ring kernels of
// nearfield_simple.hip and the general kernel of nearfield_general.hip are compiled with, and what nearfield.hip
// fill_nf_args hands the narrow ring instantiation.  Runs without a GPU.
//
//   synth_staging
//
// Output, one `key=value` per line:
//   narrow_pitch_N, narrow_cap_N   N = 1 ... 4: complex between staged blocks and blocks per round of the narrow ring
//                                  instantiation for a lens whose widest narrow collection has N order slots
//   narrow_slots_max               the order slots up to which a collection is the narrow instantiation's
//   wide_cap                       blocks per round of the wide ring instantiation
//   wide_slots_per_pass_N          N = 1 ... wide_cap: order slots per pass of a round of N blocks (UPP_TABLE's nibbles)
//   wide_slots_max                 the longest order list of a simple collection (slots lo ... hi)
//   general_cap, general_chunk     blocks per round and orders per staging pass of the general kernel
//   centre_types                   cell types per staged centre block
// Build + run:  make -C tools synth_staging && tools/synth_staging
#include <cstdio>

#include "synth_staging.h"

using namespace ml;

int main() {
    for (int n = 1; n <= SIMPLE_NARROW_SLOTS; ++n) {
        printf("narrow_pitch_%d=%d\n", n, narrow_pitch(n));
        printf("narrow_cap_%d=%d\n", n, narrow_cap(narrow_pitch(n)));
    }
    printf("narrow_slots_max=%d\n", SIMPLE_NARROW_SLOTS);
    printf("wide_cap=%d\n", SK_SLOTS);
    for (int n = 1; n <= SK_SLOTS; ++n) printf("wide_slots_per_pass_%d=%u\n", n, (UPP_TABLE >> (4 * (n - 1))) & 15u);
    printf("wide_slots_max=%d\n", SIMPLE_MAX_SLOTS);
    printf("general_cap=%d\n", NF_SLOTS);
    printf("general_chunk=%d\n", NF_CHUNK);
    printf("centre_types=%d\n", SK_TYPES);
    return 0;
}
