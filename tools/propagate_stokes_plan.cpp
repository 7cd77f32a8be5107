// The plan of the Stokes records of a propagated image (csrc/propagate_stokes.h) for given shapes, on the host:
//   propagate_stokes_plan mx my n_radii [mx my n_radii ...]
//        -> per shape a line  mx=... my=... P=... chunk=... chunks=... last=... record_doubles=... partial_doubles=...
//           (the cut is that of the focus metrics: chunk targets per chunk, last: targets of the plane's last chunk)
//   propagate_stokes_plan layout n_radii
//        -> peak_i=... peak_index=... sums=... centre=... enc=... components=... record_doubles=... radii_max=...
//   propagate_stokes_plan check have_result have_stokes T sets source mx my planes dx dy record_doubles centre [radius ...]
//        -> ok=1, or refused=-1 (an argument) / refused=-2 (the state) followed by the message on a line of its own;
//           centre: "none" (NULL), or "ci,cj" for every plane
#include <cstdlib>
#include <cstring>
#include <vector>

#include "propagate_stokes.h"

int main(int argc, char **argv) {
    using namespace ml;
    if (argc == 3 && !strcmp(argv[1], "layout")) {
        const int K = atoi(argv[2]);
        if (K < 0 || K > STOKES_RADII_MAX) {
            fprintf(stderr, "layout: 0 <= n_radii <= %d\n", STOKES_RADII_MAX);
            return 2;
        }
        printf("peak_i=%d peak_index=%d sums=%d centre=%d enc=%d components=%d record_doubles=%d radii_max=%d\n", STOKES_PEAK_I,
               STOKES_PEAK_INDEX, STOKES_SUMS, STOKES_CENTRE, STOKES_ENC, STOKES_COMPONENTS, stokes_record_doubles(K), STOKES_RADII_MAX);
        return 0;
    }
    if (argc >= 14 && !strcmp(argv[1], "check")) {
        StokesState s;
        s.have_result = atoi(argv[2]) != 0;
        s.have_stokes = atoi(argv[3]) != 0;
        s.T = atoi(argv[4]);
        s.result_sets = atoi(argv[5]);
        const int source = atoi(argv[6]), mx = atoi(argv[7]), my = atoi(argv[8]), planes = atoi(argv[9]);
        const double dx = atof(argv[10]), dy = atof(argv[11]);
        const int record_doubles = atoi(argv[12]);
        std::vector<double> centre, radii;
        if (strcmp(argv[13], "none")) {
            const char *comma = strchr(argv[13], ',');
            if (!comma || planes < 1 || planes > 4096) {
                fprintf(stderr, "check: centre is \"none\" or ci,cj (1 <= planes <= 4096)\n");
                return 2;
            }
            for (int p = 0; p < planes; ++p) {
                centre.push_back(atof(argv[13]));
                centre.push_back(atof(comma + 1));
            }
        }
        for (int i = 14; i < argc; ++i) radii.push_back(atof(argv[i]));
        char why[320];
        const int rc = stokes_check(s, source, mx, my, planes, dx, dy, centre.empty() ? nullptr : centre.data(),
                                    radii.empty() ? nullptr : radii.data(), (int)radii.size(), record_doubles, why, sizeof why);
        if (rc != 0)
            printf("refused=%d\n%s\n", rc, why);
        else
            printf("ok=1\n");
        return 0;
    }
    if (argc < 4 || (argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: propagate_stokes_plan mx my n_radii [...] | layout n_radii | check have_result have_stokes T sets source mx my "
                        "planes dx dy record_doubles centre [radius ...]\n");
        return 2;
    }
    for (int i = 1; i + 2 < argc; i += 3) {
        const int mx = atoi(argv[i]), my = atoi(argv[i + 1]), K = atoi(argv[i + 2]);
        if (mx < 1 || my < 1 || (long long)mx * my > (1 << 26) || K < 0 || K > STOKES_RADII_MAX) {
            fprintf(stderr, "mx, my >= 1, mx my <= 2^26, 0 <= n_radii <= %d\n", STOKES_RADII_MAX);
            return 2;
        }
        const long long P = (long long)mx * my, chunk = focus_chunk_targets(P);
        const int chunks = focus_chunks(P);
        printf("mx=%d my=%d P=%lld chunk=%lld chunks=%d last=%lld record_doubles=%d partial_doubles=%d\n", mx, my, P, chunk, chunks,
               P - (chunks - 1) * chunk, stokes_record_doubles(K), STOKES_PARTIAL);
    }
    return 0;
}
