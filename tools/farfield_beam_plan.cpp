// The plan of the beam metrics of a far-field map (csrc/farfield_beam.h) for given direction counts, on the host:
//   farfield_beam_plan n [n ...]
//        -> per count a line  n=... chunk=... chunks=... steps=... last=... finish_tile=... finish_tiles=... last_tile=... roundings=...
//           (chunk: directions per chunk; steps: terms a lane adds in a full chunk; last: directions of the map's last chunk;
//           of the last launch: partial records per tile, tiles, records of the last tile; roundings: beam_bound_roundings)
//   farfield_beam_plan layout
//        -> peak_p=... peak_index=... finite=... mom=... centre=... k=... cone=... record=... partial=... partial_cone=... cones_max=... slots=...
//   farfield_beam_plan check projected scattered n pair_list acc_n acc_pair_list source slot centre [cone ...]
//        -> ok=1, or refused=-1 (an argument) / refused=-2 (the state) followed by the message on a line of its own;
//           centre: "peak", or "cx,cy"; a single cone argument "null:K" passes cones = NULL with n_cones = K
//   farfield_beam_plan slots first_slot n_slots
//        -> ok=1 or refused=-1 and the message (the checks of ml_farfield_beams)
#include <cstdlib>
#include <cstring>
#include <vector>

#include "farfield_beam.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 2 && !strcmp(argv[1], "layout")) {
        printf("peak_p=%d peak_index=%d finite=%d mom=%d centre=%d k=%d cone=%d record=%d partial=%d partial_cone=%d cones_max=%d "
               "slots=%d\n", BEAM_PEAK_P, BEAM_PEAK_INDEX, BEAM_FINITE, BEAM_MOM, BEAM_CENTRE, BEAM_K, BEAM_CONE, BEAM_RECORD,
               BEAM_PARTIAL, BEAM_PARTIAL_CONE, BEAM_CONES_MAX, BEAM_SLOTS);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "slots")) {
        char why[320];
        if (beams_check(atoi(argv[2]), atoi(argv[3]), why, sizeof why) != 0)
            printf("refused=-1\n%s\n", why);
        else
            printf("ok=1\n");
        return 0;
    }
    if (argc >= 11 && !strcmp(argv[1], "check")) {
        BeamState s;
        s.projected = atoi(argv[2]) != 0;
        s.scattered = atoi(argv[3]) != 0;
        s.n = atoll(argv[4]);
        s.pair_list = atoi(argv[5]) != 0;
        s.acc_n = atoll(argv[6]);
        s.acc_pair_list = atoi(argv[7]) != 0;
        const int source = atoi(argv[8]), slot = atoi(argv[9]);
        std::vector<double> centre, cones;
        if (strcmp(argv[10], "peak")) {
            const char *comma = strchr(argv[10], ',');
            if (!comma) {
                fprintf(stderr, "check: centre is \"peak\" or cx,cy\n");
                return 2;
            }
            centre.push_back(atof(argv[10]));
            centre.push_back(atof(comma + 1));
        }
        int n_cones = 0;
        bool null_cones = false;
        if (argc == 12 && !strncmp(argv[11], "null:", 5)) {
            null_cones = true;
            n_cones = atoi(argv[11] + 5);
        } else {
            for (int i = 11; i < argc; ++i) cones.push_back(atof(argv[i]));
            n_cones = (int)cones.size();
        }
        char why[320];
        const int rc = beam_check(s, source, centre.empty() ? nullptr : centre.data(), null_cones || cones.empty() ? nullptr : cones.data(),
                                  n_cones, slot, why, sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1\n");
        return 0;
    }
    if (argc < 2) {
        fprintf(stderr, "usage: farfield_beam_plan n [...] | layout | check projected scattered n pair_list acc_n acc_pair_list source slot "
                        "centre [cone ...] | slots first_slot n_slots\n");
        return 2;
    }
    for (int i = 1; i < argc; ++i) {
        const long long n = atoll(argv[i]);
        if (n < 1 || n > BEAM_DIRECTIONS_MAX) {
            fprintf(stderr, "1 <= n <= %lld\n", BEAM_DIRECTIONS_MAX);
            return 2;
        }
        const long long chunk = beam_chunk_directions(n);
        const int chunks = beam_chunks(n), tiles = beam_finish_tiles(n);
        printf("n=%lld chunk=%lld chunks=%d steps=%d last=%lld finish_tile=%d finish_tiles=%d last_tile=%d roundings=%d\n", n, chunk,
               chunks, beam_steps(n), n - (chunks - 1) * chunk, BEAM_FINISH_TILE, tiles, beam_finish_tile_chunks(chunks, tiles - 1),
               beam_bound_roundings(n));
    }
    return 0;
}
