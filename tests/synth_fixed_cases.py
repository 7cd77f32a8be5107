"""The lenses and windows of the fixed-shape synthesis kernels' tests (csrc/nearfield_simple.hip FIXED3; csrc/lens_pack.h
fixed3_takes decides which launch takes them): test_synth_fixed_route.py holds the predicate to them and the census of
synth_cases.py to the paths each window claims, test_gpu_synth_fixed.py runs them on the GPU.  Plain data and pure
functions, no test collects from here.

The lenses are the 20 um NA 0.94 lenses of synth_cases.py - four ring collections of 1, 3, 6 and 14 rings from the
switch radius outwards, table axes of 33 nodes - with THREE order slots, all present, in every collection and in the
centre table, so that the narrow ring instantiation's round holds eight blocks (pitch 49).  What a patch meets depends
on the rings and the tables' axes, not on the order lists: the windows are those synth_cases.py found for its lens of
capacity eight."""
import synth_cases
from synth_cases import NA, O2, O3, RADIUS, SPAN_DEG, U_STEPS, Lens, ox

O3_LOW = ox(-2, -1, 0)
O3_HOLE = ox(-1, 1)                         # three slots from -1, the middle one a hole: present = 0b101
# every collection (-1, 0, 1): neighbouring collections share their lowest order
LENS_F3 = Lens(RADIUS, NA, U_STEPS, SPAN_DEG, (O3,), O3)
# collections 0 ... 3: lowest order -2, -1, -2, -1 - neighbouring collections differ in it
LENS_F3_LO = Lens(RADIUS, NA, U_STEPS, SPAN_DEG, (O3_LOW, O3), O3)
# one collection of two slots among them (collection 1): the general kernels for the whole lens' rings
LENS_ONE_TWO_SLOT = Lens(RADIUS, NA, U_STEPS, SPAN_DEG, (O3, O2, O3, O3), O3)

# name -> (case, the paths it claims).  Claims: tags of synth_cases.TAGS, confirmed by synth_cases.confirm, and
#   'two-collections-equal-lo'   a patch with ring samples of two collections whose lists are the same
#   'ring-and-centre'            a patch with ring samples and centre samples: both kernels store into it
_S = synth_cases.SIMPLE
CASES = {
    # across collections 1, 2 and 3: a patch of exactly eight blocks, second and third rounds, two collections of
    # different lowest order in a wave, partial patches on both far sides
    'mid-lo': (synth_cases._case(LENS_F3_LO, (0.5, 20), (43, 37), 'x', _S, ()), (
        'narrow:round-exactly-capacity', 'narrow:second-round-capacity-8', 'narrow:third-round',
        'narrow:two-collections-in-a-wave', 'narrow:multi-round-partial-patches')),
    # the same radii at another azimuth (a new geometry for the library: its first synthesis runs over the whole grid),
    # every collection the same list
    'mid-equal': (synth_cases._case(LENS_F3, (0.5, 65), (43, 37), 'y', _S, ()), (
        'narrow:second-round-capacity-8', 'two-collections-equal-lo')),
    # the rim: five to six rings per patch, whole patches only (a third round there on one or two patches only, fewer
    # than the census' margin: the third round is the mid-radius windows' claim)
    'rim': (synth_cases._case(LENS_F3_LO, (0.93, 45), (48, 40), 'z', _S, ()), (
        'narrow:second-round-capacity-8', 'narrow:slots-3')),
    # across the switch radius (0.15 of the lens radius): ring and centre kernels store into the same patches
    'switch': (synth_cases._case(LENS_F3, (0.15, 0), (43, 37), 'x', _S, ()), (
        'ring-and-centre', 'narrow:slots-3')),
}
# launches of the same windows that keep the general kernels: (lens, window of CASES, source_z in focal distances or
# None = a plane wave)
OTHERS = {
    'plane-wave': (LENS_F3, 'mid-equal', None),
    'two-slot-collection': (LENS_ONE_TWO_SLOT, 'mid-equal', 1.0),
}
BATCH_CASE = 'mid-lo'   # also run as a three-polarisation batch


def patches_with_ring_and_centre(args):
    """8 x 8 patches that hold ring samples and centre samples, by the oracle's decisions"""
    import numpy as np
    from oracle import nearfield_oracle
    dec = {}
    nearfield_oracle.build_nearfield(decisions=dec, **args)
    ring, centre = dec['which_gc'] >= 0, np.asarray(dec['in_center'], dtype=bool)
    nx, ny = ring.shape
    return sum(1 for bi in range((nx + 7) // 8) for bj in range((ny + 7) // 8)
               if ring[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8].any() and centre[8 * bi:8 * bi + 8, 8 * bj:8 * bj + 8].any())


def confirm(cen, args, claim):
    """the number of patches that meet a claim of CASES"""
    if claim == 'two-collections-equal-lo':
        K = cen.colls
        return sum(1 for p in cen.patches
                   if len(p.blocks) >= 2 and len({(K[c].n_slots, K[c].lo, K[c].present) for c in p.blocks}) == 1)
    if claim == 'ring-and-centre':
        return patches_with_ring_and_centre(args)
    return synth_cases.confirm(cen, claim)
