// Which form of the synthesis kernels a launch takes - the fixed-shape kernels of three-order tables or the general
// ones (metalens_amd/csrc/lens_pack.h fixed3_takes) - for a lens as tools/lens_pack lays it out and the facts of a
// launch.  Runs without a GPU.
//
//   synth_fixed_route PACKED N_POL USE_ACTIVE FIRST_PASS PLANE_WAVE PREMOD
//
// PACKED is the OUT file of tools/lens_pack (the record format: lens_pack.cpp); read from it are coll (CollDesc[]),
// narrow_mask, center_n_slots, center_present_mask and table_desc (the centre table's descriptor is its last).  The five
// numbers are Fixed3Facts' launch part.  Prints, as key=value words, what the lens' tables allow (lens_ring,
// lens_centre) and what this launch takes (ring, centre).
// Build + run:  make -C tools synth_fixed_route && tools/synth_fixed_route lens.out 1 1 0 0 0
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "lens_pack.h"

using namespace ml;

int main(int argc, char **argv) {
    if (argc != 7) return fprintf(stderr, "usage: %s PACKED N_POL USE_ACTIVE FIRST_PASS PLANE_WAVE PREMOD\n", argv[0]), 2;
    std::map<std::string, std::vector<char>> in;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return perror(argv[1]), 2;
    char name[128], type[8];
    size_t count;
    while (fscanf(f, "%127s %7s %zu", name, type, &count) == 3) {
        const size_t item = type[1] - '0';
        std::vector<char> &r = in[name];
        r.resize(count * item);
        if (fgetc(f) != '\n' || (count && fread(r.data(), item, count, f) != count) || fgetc(f) != '\n')
            return fprintf(stderr, "%s: record %s is cut short\n", argv[1], name), 2;
    }
    fclose(f);
    for (const char *need : {"coll", "narrow_mask", "center_n_slots", "center_present_mask", "table_desc"})
        if (!in.count(need)) return fprintf(stderr, "%s: no record %s\n", argv[1], need), 2;
    auto word = [&in](const char *n) { return *reinterpret_cast<const int32_t *>(in[n].data()); };
    if (in["coll"].size() % sizeof(CollDesc) || in["coll"].size() > MAX_RING_COLLS * sizeof(CollDesc) ||
        in["table_desc"].size() != (MAX_SLOTS + 1) * sizeof(TableDesc))
        return fprintf(stderr, "%s: coll or table_desc has another size than the records of lens_pack.h\n", argv[1]), 2;
    CollDesc coll[MAX_RING_COLLS] = {};
    memcpy(coll, in["coll"].data(), in["coll"].size());
    TableDesc centre;
    memcpy(&centre, in["table_desc"].data() + MAX_SLOTS * sizeof(TableDesc), sizeof centre);
    Fixed3Facts facts = {coll, word("narrow_mask"), word("center_n_slots"), word("center_present_mask"), centre.uniform,
                         atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])};
    const Fixed3 lens = fixed3_lens(facts), takes = fixed3_takes(facts);
    printf("lens_ring=%d lens_centre=%d ring=%d centre=%d\n", (int)lens.ring, (int)lens.centre, (int)takes.ring, (int)takes.centre);
    return 0;
}
